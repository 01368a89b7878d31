"""The cases of the entropy decoder's branches (tests/hzdec_plan.py): hand-written plane payloads.

A payload is the reference's plane framing (hzcc.c:449-476) around a chain  U(run_1) | U(run_2) N(v_1) | ... | N(v_n)  built
pair by pair, so that a case can put a chosen bit of a chosen code on a chosen boundary: pad with short pairs (3 and 5 bits) up
to the bit before, then place a probe pair whose bits run through all five machine states.  The model reports what a payload
reaches; every case names the labels it is there for and tests/test_hzdec_plan_host.py checks them.

Every payload is one on which the reference terminates inside the buffer: all announced codes are present, or `len` cuts into a
chain that goes on behind it (at least 16 bytes, except where the cut is in the final code, behind which the plane ends); every
buffer ends in GUARD bytes of 0xFF; runs stay at or below 2^31 - 2 and value x quantiser inside an int.

  * OP_CASES   -- one plane through dsvg_op_decode_plane against orc_decode_plane (the int32 path), quantiser OP_Q, hz_cases.op_stab;
  * pipe_planes -- hand-built planes for the pipeline seam, spliced into real packets by tests/test_gpu_hzdec_paths.py.
"""
import ctypes as C

import numpy as np

import _cabi as A
import hz_cases as HC
import hz_plan as H
import hzdec_plan as D
from _hzbits import BW, splice

OP_Q = HC.OP_Q
GUARD = 32
WIDE = (512, 288)                # nscan 147456: room for a kept run of 131071 and more (a run code of 35 bits)
CIF = (352, 288)                 # nscan 101376: room for runs of 65535 and more, 8192 entries and three passes of 131072 bits
PROBE = (2, 3)                   # U(2) N(3) = 011 011s: bits 0..6 are entered in states 0 1 0 2 3 2 4
PROBE_AT = {0: 0, 1: 1, 2: 3, 3: 4, 4: 6}          # state -> the probe's bit that must sit on the boundary


class Chain:
    """run_1, the pairs (run_{m+1}, v_m) in payload order, the final value; bits = chain bits behind U(run_1) so far"""

    def __init__(self, run1=0, seed=1):
        self.run1, self.pairs, self.bits, self.final = run1, [], 0, 1
        self.rng = np.random.default_rng(seed)

    def add(self, run, v):
        self.pairs.append((run, v))
        self.bits += H.len_ueg(run) + H.len_neg(v)
        return self

    def short(self, nbits):
        """one short pair of 3 or 5 bits: run 0, value +-1 / +-2, +-3"""
        s = -1 if self.rng.integers(2) else 1
        return self.add(0, s if nbits == 3 else s * int(self.rng.integers(2, 4)))

    def pad_to(self, target):
        """short pairs up to exactly `target` chain bits"""
        left = target - self.bits
        assert left in (0, 3, 5, 6) or left >= 8, "cannot pad %d bits with pairs of 3 and 5" % left
        while left > 12:
            k = 3 if self.rng.integers(2) else 5
            self.short(k)
            left -= k
        for k in {0: (), 3: (3,), 5: (5,), 6: (3, 3), 8: (3, 5), 9: (3, 3, 3), 10: (5, 5), 11: (3, 3, 5), 12: (3, 3, 3, 3)}[left]:
            self.short(k)
        assert self.bits == target
        return self

    def probe(self, boundary, state):
        """the probe pair placed so that chain bit `boundary` is entered in `state`"""
        return self.pad_to(boundary - PROBE_AT[state]).add(*PROBE)

    @property
    def n(self):
        return len(self.pairs) + 1


def payload(dc, chain, announced=None, guard=GUARD):
    """(buffer, plen, S0): the bytes behind a plane's length word -- SEG(DC), the announced count, the chain, the end-of-plane
    symbol (plen counts up to here), guard bytes; chain None: a plane without entries"""
    a = BW()
    a.seg(dc)
    a.align()
    a.put(32, chain.n if announced is None else announced)
    s0 = None
    if chain is not None:
        a.ueg(chain.run1)
        s0 = a.nbits
        for run, v in chain.pairs:
            a.ueg(run)
            a.neg(v)
        a.neg(chain.final)
        assert a.nbits == s0 + chain.bits + H.len_neg(chain.final)
    a.align()
    a.put(8, 0x55)
    out = a.bytes()
    return out + b"\xff" * guard, len(out), s0


HEAD = 40                         # SEG of a small DC fills one byte, the count four: U(run_1) starts at bit 40


def s0_of(run1):
    return HEAD + H.len_ueg(run1)


# ---------------------------------------------------------------------------------------------------------------------------
def _case(w, h, dc, chain, labels, length=None, announced=None):
    buf, plen, s0 = payload(dc, chain, announced=0 if chain is None and announced is None else announced)
    return dict(w=w, h=h, buf=buf, len=plen if length is None else length, plen=plen, labels=labels)


def _cut_cases(out):
    """len at every bit phase of the last bit of a value (42 short pairs in, 100 and more behind) and of the final code's sign bit"""
    for ph in range(8):
        # a value in mid-chain
        ch = Chain(1, seed=10 + ph)
        t = 300
        while (s0_of(1) + t - 1) % 8 != ph:
            t += 1
        ch.pad_to(t - 5).add(0, -2 if ph & 1 else 3)       # the target pair: U(0) N(+-2 / 3), 5 bits, its last bit at chain bit t-1
        ch.pad_to(t + 400)
        x = (s0_of(1) + t - 1) >> 3
        for k, ln in (("a", x), ("b", x + 1)):
            lab = []
            if ln == x + 1:
                lab = ["cd.cut.val.kept"] if ph == 6 else ["cd.cut.val.flush"] if ph == 7 else []
            elif ph == 0:
                lab = ["cd.cut.val.next"]
            lab += {(0, "a"): ["pa.short.even"], (1, "a"): ["pa.short.odd"]}.get((ph, k), [])      # (codes found before the cut: the model counts them)
            out["cut-val-%d%s" % (ph, k)] = _case(64, 64, 2, ch, lab, length=ln)
        # the final code
        ch = Chain(1, seed=30 + ph)
        ch.final = -2 if ph & 1 else 2                      # N(+-2): 4 bits
        t = 300
        while (s0_of(1) + t + 4 - 1) % 8 != ph:
            t += 1
        ch.pad_to(t)
        x = (s0_of(1) + t + 3) >> 3
        for k, ln in (("a", x), ("b", x + 1)):
            lab = []
            if ln == x + 1:
                lab = ["cd.cut.last.kept"] if ph == 6 else ["cd.cut.last.flush"] if ph == 7 else []
            elif ph == 0:
                lab = ["cd.cut.last.next"]
            out["cut-last-%d%s" % (ph, k)] = _case(64, 64, -2, ch, lab, length=ln)


def _shared(w, h, level):
    """(earlier position, later position) of a cell that a region of scan level `level` shares with one of the next level"""
    seen = {}
    for p in range(H.geometry(w, h)[0], H.geometry(w, h)[1]):
        x, y, lv = H.cell_of(w, h, p)
        if (x, y) in seen and lv == level + 1 and H.cell_of(w, h, seen[(x, y)])[2] == level:
            return seen[(x, y)], p
        seen.setdefault((x, y), p)
    raise AssertionError("no shared cell")


def from_entries(run1_entries, seed=1):
    """a chain from [(scan position, value)] in scan order"""
    ch = Chain(run1_entries[0][0], seed)
    for (p0, v0), (p1, v1) in zip(run1_entries, run1_entries[1:]):
        ch.add(p1 - p0 - 1, v0)
    ch.final = run1_entries[-1][1]
    return ch


OVERLAP = (20, 30) if H.overlaps(20, 30) else (250, 130)
_cases = {}


def op_cases():
    """name -> dict(w, h, buf, len, plen, labels)"""
    if _cases:
        return _cases
    out = _cases
    W, Hh = CIF
    nscan = H.geometry(W, Hh)[1]
    r = H.regions(64, 64)
    # --- the head
    out["runs0"] = _case(8, 8, 5, None, ["pa.runs0"])
    out["runs-neg"] = _case(8, 8, -5, None, ["pa.runs_neg"], announced=0x80000005)
    ch = Chain(1, 2)
    for i in range(2999):
        ch.add(0, (i % 5) - 2 or 1)
    out["runs-clamped"] = _case(8, 8, 1, ch, ["pa.runs_clamped", "pa.all_found", "po.last_cell", "po.nscan", "po.vec"])
    ch = Chain(5)
    ch.final = -3
    out["n1"] = _case(8, 8, 0, ch, ["cd.last.n1", "po.tail", "pa.pass1", "cd.last.sign.same", "po.pass1"])
    # an entry at position 0 (the DC's cell), one in the LL region, one in each level group
    out["pos0"] = _case(64, 64, -9, from_entries([(0, 7), (3, -2), (r[1][0] + 5, 4), (r[4][0] + 9, -1), (r[7][0] + 100, 6), (r[9][0] + 1000, -3)]),
                        ["sc.pos0", "sc.ll", "sc.lv0", "sc.lv1", "sc.lv2", "pa.u1.len1"])
    out["pos0-alone"] = _case(8, 8, 11, from_entries([(0, -4)]), ["sc.pos0", "cd.last.n1"])
    ch = Chain(2, 3).pad_to(600)
    out["announced-fewer"] = _case(64, 64, 4, ch, ["pa.all_found"], announced=20)
    # --- long codes
    # (a U part of 33 bits has its 32 body bits in one 32-bit word, where the short decoder happens to be right as well: 35 bits
    # and more, with data bits that are not all zero, tell the two apart -- a kept run of 131071 or more needs WIDE's larger scan)
    out["long-run1"] = _case(*WIDE, 3, from_entries([(140000, 5), (140001, -200001), (140010, 0x5A5A5A), (140011, -(1 << 20)), (140500, 2)]),
                             ["pa.u1.gt31", "cd.val.u63", "cd.val.u31", "cd.run.u31"])
    out["long-run"] = _case(*WIDE, 3, from_entries([(3, 5), (140004, -7), (140005, 65537), (140006, -0x6B3C5), (147000, 1)]), ["cd.run.u63", "cd.val.u63"])
    out["long-33"] = _case(W, Hh, 3, from_entries([(3, 5), (70004, -7), (70005, 65537), (70006, -65536), (70007, 1)]), ["cd.run.u63", "cd.val.u63"])
    big = (1 << 31) - 2
    ch = Chain(5, 4).add(big, 3).add(big, -2)
    for i in range(12):
        ch.add(i % 3, i - 20)
    out["sum64"] = _case(W, Hh, 1, ch, ["po.sum64", "cd.run.u63"])
    ch = Chain(1 << 30, 4).add(0, 3).add(1 << 30, -2).add(0, 1)
    out["run1-2^30"] = _case(W, Hh, 1, ch, ["pa.u1.gt31"])
    out["edge-cells"] = _case(W, Hh, -1, from_entries([(nscan - 2, 9), (nscan - 1, -8), (nscan, 7), (nscan + 1, 6)]), ["po.last_cell", "po.nscan", "pa.u1.gt31"])
    # --- cuts
    _cut_cases(out)
    ch = Chain(70000, 5).pad_to(400)
    out["cut-header"] = _case(W, Hh, 3, ch, ["pa.u1.w0", "pa.u1.cut"], length=5)
    out["cut-u1"] = _case(W, Hh, 3, ch, ["pa.u1.cut"], length=7)
    ch = Chain(1, 6).pad_to(3000)
    s0 = s0_of(1)
    out["cut-first-chunk-lt64"] = _case(64, 64, 3, ch, ["pa.end.keep_lt64", "pa.m1_empty", "pa.end.past"], length=12)
    out["cut-first-chunk-gt64"] = _case(64, 64, 3, ch, ["pa.end.keep_gt64"], length=16)
    edge = (s0 + 3 * 128 + 7) >> 3                          # the first byte boundary at or past chunk 3's first bit: 1..7 bits of it are data
    out["cut-chunk-edge-over"] = _case(64, 64, 3, ch, ["pa.end.keep_lt64"], length=edge)
    out["cut-chunk-edge-under"] = _case(64, 64, 3, ch, ["pa.end.keep_gt64"], length=edge - 1)
    # a long run code cut in its middle: the chunk it lies in has no code end at all
    # (the code fills chain bits 354..414, chunk 3 begins at 384, the data ends 9..16 bits into it)
    ch = Chain(1, 7).pad_to(354).add(big, 2).pad_to(354 + 61 + 4 + 300)
    out["cut-no-end"] = _case(64, 64, 3, ch, ["pa.m_none", "pa.end.keep_lt64"], length=(s0 + 3 * 128 + 16) >> 3)
    # --- states on chunk and wave boundaries; the chunk's bit 64 as a code start; more than 8192 entries
    ch = Chain(0, 8)
    for k, st in enumerate((0, 1, 2, 3, 4)):
        ch.probe(128 * (k + 1), st)
    ch.pad_to(128 * 7 + 64).add(*PROBE)                     # a code from bit 64 of chunk 7
    for k, st in enumerate((0, 1, 2, 3, 4)):
        ch.probe(128 * 64 * (k + 1), st)
    ch.pad_to(128 * 64 * 5 + 3000)
    out["states"] = _case(W, Hh, 2, ch, ["pa.chunk.s%d" % s for s in range(5)] + ["pa.wave.s%d" % s for s in range(5)] + [
        "pa.straddle.chunk", "pa.straddle.wave", "cd.start.w0.al", "cd.start.w0.un", "cd.start.w1.al", "cd.start.w1.un", "cd.start.prev.un",
        "po.pass2", "po.vec", "pa.pass1", "pa.u1.len1"])
    # --- passes: every state carried into a pass; a cut on either side of a pass boundary
    P = D.PASS_BITS
    ch = Chain(0, 9).probe(P, 1).probe(2 * P, 2).pad_to(2 * P + 500)
    out["pass-s1-s2"] = _case(W, Hh, 2, ch, ["pa.pass3", "pa.pass.s1", "pa.pass.s2", "pa.straddle.pass"])
    ch = Chain(0, 10).probe(P, 3).probe(2 * P, 4).pad_to(2 * P + 500)
    out["pass-s3-s4"] = _case(W, Hh, -2, ch, ["pa.pass3", "pa.pass.s3", "pa.pass.s4", "pa.straddle.pass"])
    ch = Chain(0, 11).probe(P, 0).pad_to(P + 1000)
    out["pass-s0"] = _case(W, Hh, 2, ch, ["pa.pass2", "pa.pass.s0", "cd.start.w0.al"])
    s0 = s0_of(0)
    edge = (s0 + P + 7) >> 3
    out["cut-pass-edge-over"] = _case(W, Hh, 2, ch, ["pa.pass2", "pa.end.keep_lt64"], length=edge)
    out["cut-pass-edge-under"] = _case(W, Hh, 2, ch, ["pa.pass1", "pa.end.keep_gt64"], length=edge - 1)
    # --- the final code's sign bit behind a chunk and behind a pass: its U part (3 bits, N(2) = 001s) ends on the boundary
    ch = Chain(0, 12).pad_to(128 * 3 - 3)
    ch.final = -2
    out["last-sign-chunk"] = _case(64, 64, 2, ch, ["cd.last.sign.chunk"])
    ch = Chain(0, 13).pad_to(P - 3)
    ch.final = -2
    out["last-sign-pass"] = _case(W, Hh, 2, ch, ["cd.last.sign.pass", "pa.pass1"])
    # --- cells two regions share
    w, h = OVERLAP
    for lv in (0, 1):
        e, l = _shared(w, h, lv)
        out["shared-both-%d%d" % (lv, lv + 1)] = _case(w, h, 6, from_entries(sorted([(2, 3), (e, 5), (e + 1, -1), (l, -7), (l + 2, 2)])), ["sc.shared.%d%d.both" % (lv, lv + 1)])
        out["shared-earlier-%d%d" % (lv, lv + 1)] = _case(w, h, 6, from_entries(sorted([(2, 3), (e, 5), (e + 1, -1), (l + 2, 2)])), ["sc.shared.%d%d.earlier" % (lv, lv + 1)])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline seam: planes to splice into real packets (all planes of a 4:4:4 picture have the picture's size)
PIPE_G = (352, 288, A.SUBSAMP_444)


POS0_DC, POS0_SYM, POS0_SEED = -400000, 7, 0xDEC0


def pipe_plane(name, w=PIPE_G[0], h=PIPE_G[1]):
    """dict(w, h, buf (the plane's bytes up to its end-of-plane symbol), plen) of a w x h coefficient plane"""
    r = H.regions(w, h)
    if name in ("pos0", "pos0-dc-lost"):
        # entry 1 on the DC's cell, then one entry in the LL region and in each level group.  The DC is large enough for every sample
        # of the decoded plane to depend on it (a DC of a few thousand vanishes in nine levels' rounding); "pos0-dc-lost" is what a
        # scatter would decode in which entry 1 wins the cell: the same plane with entry 1's symbol as its DC
        c = _case(w, h, POS0_DC if name == "pos0" else POS0_SYM, from_entries([(0, POS0_SYM), (5, 3), (r[2][0] + 4 * r[2][3] + 9, -2), (r[5][0] + 3 * r[5][3] + 7, 1), (r[8][0] + 10 * r[8][3] + 10, 1)]), [])
    elif name == "empty":
        c = _case(w, h, -7, None, [])
    elif name == "sparse":
        c = _case(w, h, 4, from_entries([(3, 2), (r[4][0] + 2 * r[4][3] + 1, -1), (r[7][0] + 5 * r[7][3] + 2, 1)]), [])
    elif name == "three-pass":
        c = op_cases()["pass-s1-s2"]
        assert (c["w"], c["h"]) == (w, h)
    else:
        raise ValueError(name)
    return dict(w=w, h=h, buf=c["buf"][:c["plen"]], plen=c["plen"])


def _lens(*names):
    return [pipe_plane(n)["plen"] for n in names]


# name -> kinds of the call's jobs, symbol path or int32, the planes spliced in, the labels the call is there for
PIPE_CALLS = {
    "pos0-luma": dict(kinds="PP", sym=True, planes=[pipe_plane("pos0")], labels=["sc.pos0", "sc.sym", "cl.sym", "la.scatter1"]),
    "pos0-chroma": dict(kinds="PP", sym=True, planes=[pipe_plane("pos0")], labels=["sc.pos0", "sc.sym"]),
    "unequal": dict(kinds="PP", sym=True, planes=[pipe_plane("empty"), pipe_plane("three-pass")], lens=_lens("empty", "three-pass"),
                    labels=["la.unequal", "la.scatter1", "pa.runs0", "pa.pass3"]),
    "unequal-i32": dict(kinds="PP", sym=False, planes=[pipe_plane("empty"), pipe_plane("three-pass")], lens=_lens("empty", "three-pass"),
                        labels=["la.unequal", "la.scatter3", "sc.i32", "cl.vec"]),
    "i-and-p": dict(kinds="PI", sym=True, planes=[pipe_plane("pos0")], labels=["la.ip", "la.scatter1"]),
    "i-and-p-i32": dict(kinds="PI", sym=False, planes=[pipe_plane("pos0")], labels=["la.ip", "la.scatter3"]),
    # DSV1_NO_DEC_SYM_I: the I picture keeps int32 coefficients beside a P picture on the symbol path
    "i-and-p-mixed": dict(kinds="PI", sym=True, sym_i=False, planes=[pipe_plane("pos0")], labels=["la.ip", "la.scatter3", "la.mixed"]),
    "dense-then-sparse": dict(kinds="P", sym=True, planes=[pipe_plane("three-pass"), pipe_plane("sparse")], labels=["sc.sym", "cl.sym"]),
}


_streams = {}


def base_stream(g, kinds, seed):
    """packets of an oracle stream of len(kinds) pictures of the given kinds, and the indices of its picture packets"""
    key = (g, kinds, seed)
    if key not in _streams:
        w, h, fmt = g
        clip = A.gen_clip(w, h, fmt, seed, len(kinds), style=0)
        # (scene-change detection off: the kinds are the GOP's; 'I' after the first picture by a GOP of one)
        stream, _ = A.orc_encode(clip, A.orc_cfg(w, h, fmt, qp=85, gop=1 if kinds[1:].count("I") else 12, rc_mode_cli=1, scd=0))
        pk = A.split_packets(stream)
        pics = [i for i, p in enumerate(pk) if p[5] & 4]
        assert "".join("P" if pk[i][5] & 1 else "I" for i in pics) == kinds, "the oracle coded %s" % [pk[i][5] for i in pics]
        _streams[key] = (pk, pics)
    pk, pics = _streams[key]
    return list(pk), pics


def spliced(g, kinds, seed, edits):
    """the stream's packets with edits [(picture, plane index, pipe plane name)] spliced in"""
    pk, pics = base_stream(g, kinds, seed)
    for pic, plane, name in edits:
        pl = pipe_plane(name, *A.coef_dims(g[0], g[1], g[2], plane))
        pk[pics[pic]] = splice(pk[pics[pic]], {plane: pl["buf"]})
    return pk


_models = {}


def model_of(name):
    if name not in _models:
        c = op_cases()[name]
        _models[name] = D.Plane(c["w"], c["h"], c["buf"], c["len"])
    return _models[name]


def decode(L, fn, case):
    """fn = 'orc_decode_plane' | 'dsv_decode_plane' | 'dsvg_op_decode_plane' on a copy of the case's buffer: the int32 plane"""
    w, h = case["w"], case["h"]
    st, keep = HC.op_stab(w, h)
    buf = np.frombuffer(case["buf"], dtype=np.uint8).copy()
    co = np.zeros(w * h, dtype=np.int32)
    rc = getattr(L, fn)(A.u8p(buf), case["len"], C.byref(A.Coefs(A.i32p(co), w, h)), OP_Q, C.byref(st))
    if fn.startswith("dsvg"):
        A.chk(L, rc)
    assert bytes(buf) == case["buf"], "the decoder wrote into its input"
    return co
