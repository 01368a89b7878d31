"""The average-bitrate rate control restated in plain Python integers, from the reference's side (quality2quant dsv_encoder.c:70-168,
the statistics of dsv_enc dsv_encoder.c:816-848, the declarations dsv_encoder.h:58-104, the framing of a picture packet
dsv_encoder.c:518-536 + hzcc.c:449-476, dsv_bs_put_seg bs.c:147-157, the quantiser tables hzcc.c:50-92,190-208 + sbt.c:677-696), with no
knowledge of include/dsvg_rc.h.  C's 32-bit arithmetic is spelled out: truncating signed division, unsigned division where either
operand is declared unsigned, arithmetic right shifts, wrap to 32 bits on conversion.

Every function returns the branch labels it went through, so that a test can assert that its inputs reached them all.  A signed
intermediate that leaves int32 is undefined in C: the model then sets overflow=True on its result and the callers drop the case.  States
that make the reference divide by zero (need == 0, fps_den <= 0, a bpf_reset that wraps to 0) raise ValueError: no test may feed them
to any library.

tests/test_rc_host.py holds the product's header to this model, tests/test_rc_ref.py the model to the reference library itself,
tests/test_gpu_rc_paths.py the device's compile of the header."""
import random

MAXQ = 2047                     # DSV_MAX_QUALITY dsv.h:157
BPF_RESET = 256                 # DSV_BPF_RESET dsv_encoder.h:86


def PCT(p):                     # DSV_QUALITY_PERCENT dsv.h:158
    return MAXQ * p // 100


# the sixteen words of a rate-control state: eight of state (DSV_ENCODER "used internally"), eight parameters
STATE_FIELDS = ("rc_quant", "bpf_total", "bpf_reset", "bpf_avg", "total_P_frame_q", "avg_P_frame_q", "last_P_frame_over", "back_into_range")
PARAM_FIELDS = ("bitrate", "fps_num", "fps_den", "rc_high_motion_nudge", "max_q_step", "min_quality", "max_quality", "min_I_frame_quality")
FIELDS = STATE_FIELDS + PARAM_FIELDS
UNSIGNED = ("rc_quant", "bpf_total", "bpf_reset", "bitrate")

PICK_LABELS = frozenset("""first over under nudge_down nudge_up_P nudge_up_I I_ignores_over nudge_off step_lo step_hi cap cap16 uncapped
    fi_lt60 fi_lt70 fi_lt75 fi_none fi_ceiling fi_ceiling_negative p_floor_min p_floor_max p_floor_avg floor_hit i_floor_hit ceiling_hit
    bounds_inverted final_clamp fps_zero quant_ends""".split())
AFTER_LABELS = frozenset("I_clears P_over P_under P_between P_eq_three_quarters P_eq_seven_eighths back_set wrap_I wrap_P fps_zero".split())
PACKET_LABELS = frozenset("dc0 dc_1byte_max dc_2byte_min dc_2byte_max dc_3byte_min dc_negative bits_mult8 bits_not_mult8 bits_zero".split())
ALL_LABELS = frozenset(["pick." + x for x in PICK_LABELS] + ["after." + x for x in AFTER_LABELS] + ["packet." + x for x in PACKET_LABELS])

M32 = 0xFFFFFFFF


def u32(x):
    return x & M32


def s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def tdiv(a, b):
    """C's int division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class _Ovf:
    """collects 'a signed intermediate left int32'"""
    def __init__(self):
        self.hit = False

    def __call__(self, x):
        if not -(1 << 31) <= x < (1 << 31):
            self.hit = True
            return s32(x)
        return x


def clamp(v, lo, hi):
    """the CLAMP macro (dsv.h): ((v) < (lo) ? (lo) : ((v) > (hi) ? (hi) : (v))); also says which arm was taken"""
    if v < lo:
        return lo, "lo"
    if v > hi:
        return hi, "hi"
    return v, "in"


class State(dict):
    """a rate-control state as a dict of the sixteen FIELDS, plus .overflow"""
    overflow = False

    def copy(self):
        s = State(self)
        s.overflow = self.overflow
        return s

    def words(self):
        return [u32(self[f]) for f in FIELDS]


def make_state(**kw):
    s = State((f, 0) for f in FIELDS)
    s.update(fps_num=30, fps_den=1, rc_high_motion_nudge=1, max_q_step=MAXQ // 200, min_quality=PCT(1), max_quality=PCT(95),
             min_I_frame_quality=PCT(5), bitrate=0x7FFFFFFF)          # dsv_enc_init dsv_encoder.c:696-722
    for k, v in kw.items():
        assert k in FIELDS, k
        s[k] = v
    return s


def _fps_int(st, ov):
    """fps = (fps_num << 5) / fps_den on ints (dsv_encoder.c:88 and :826)"""
    if st["fps_den"] <= 0:
        raise ValueError("fps_den <= 0: the reference divides by it")
    if st["fps_num"] < 0:
        ov.hit = True                              # left shift of a negative int
    return tdiv(ov(st["fps_num"] << 5), st["fps_den"])


def needed_bpf(st):
    """needed bytes per frame as pick sees it; raises for the states no library may be fed"""
    ov = _Ovf()
    fps = _fps_int(st, ov)
    if fps == 0:
        fps = 1
    need = s32((u32(st["bitrate"] << 5) // u32(fps)) >> 3)
    if need == 0:
        raise ValueError("need == 0: the reference divides by it")
    return need


def pick(state, isP, forced_intra):
    """quality2quant for an ABR stream -> (frame_quant, state, labels)"""
    st = state.copy()
    L = set()
    ov = _Ovf()
    q = s32(st["rc_quant"])                                    # int q = enc->rc_quant
    fps = _fps_int(st, ov)
    if fps == 0:
        fps = 1
        L.add("fps_zero")
    need = s32((u32(st["bitrate"] << 5) // u32(fps)) >> 3)     # unsigned << and /, then into an int
    if need == 0:
        raise ValueError("need == 0: the reference divides by it")
    bpf = st["bpf_avg"]
    if bpf == 0:
        bpf = need
        L.add("first")
    diff = ov(bpf - need)
    dirn = -1 if diff > 0 else 1
    L.add("over" if dirn < 0 else "under")
    if diff == -(1 << 31):
        ov.hit = True                                          # abs(INT_MIN)
    delta = tdiv(ov(abs(diff) << 9), need)
    if dirn == 1:
        delta = ov(delta * 2)
    nudged = False
    over, back = st["last_P_frame_over"] != 0, st["back_into_range"] != 0
    if st["rc_high_motion_nudge"]:
        if isP:
            if over:
                delta = ov(ov(delta + 1) * 2); dirn = -1; nudged = True
                L.add("nudge_down")
            elif back:
                delta = ov(ov(delta + 1) * 2); dirn = 1; nudged = True
                L.add("nudge_up_P")
        else:
            if back:
                delta = ov(ov(delta + 1) * 2); dirn = 1; nudged = True
                L.add("nudge_up_I")
            elif over:
                L.add("I_ignores_over")
    elif over or back:
        L.add("nudge_off")
    delta = ov(q * delta) >> 9                                 # arithmetic shift
    if st["max_q_step"] <= 0:
        L.add("step_lo")
    elif st["max_q_step"] > MAXQ:
        L.add("step_hi")
    st["max_q_step"] = clamp(st["max_q_step"], 1, MAXQ)[0]     # written back (dsv_encoder.c:129)
    cap = st["max_q_step"] * 16 if nudged else st["max_q_step"]
    if delta > cap:
        delta = cap
        L.add("cap16" if nudged else "cap")
    else:
        L.add("uncapped")
    delta = ov(delta * dirn)
    q = ov(q + delta)
    if st["min_quality"] > st["max_quality"]:
        L.add("bounds_inverted")
    low_p, arm = clamp(ov(st["avg_P_frame_q"] - PCT(4)), st["min_quality"], st["max_quality"])
    L.add({"lo": "p_floor_min", "hi": "p_floor_max", "in": "p_floor_avg"}[arm])
    minq = low_p if isP else st["min_I_frame_quality"]
    if forced_intra:
        if q < PCT(60):
            q = ov(q + PCT(15)); L.add("fi_lt60")
        elif q < PCT(70):
            q = ov(q + PCT(8)); L.add("fi_lt70")
        elif q < PCT(75):
            q = ov(q + PCT(3)); L.add("fi_lt75")
        else:
            L.add("fi_none")
        ceil = ov(st["max_quality"] - PCT(5))
        q, arm = clamp(q, 0, ceil)
        if ceil < 0:
            L.add("fi_ceiling_negative")
        elif arm == "hi":
            L.add("fi_ceiling")
    q, arm = clamp(q, minq, st["max_quality"])
    if arm == "lo":
        L.add("floor_hit" if isP else "i_floor_hit")
    elif arm == "hi":
        L.add("ceiling_hit")
    q, arm = clamp(q, 0, MAXQ)
    if arm == "hi":
        L.add("final_clamp")                                   # only a max_quality above 2047 lets q get here
    st["rc_quant"] = u32(q)
    if q in (0, MAXQ):
        L.add("quant_ends")
    fq = MAXQ - tdiv(ov((MAXQ - 5) * q), MAXQ)
    st.overflow = st.overflow or ov.hit
    return fq, st, L


def after(state, isP, pkt_len):
    """the statistics after a picture packet of pkt_len bytes -> (state, labels)"""
    st = state.copy()
    L = set()
    ov = _Ovf()
    pkt_len = u32(pkt_len)
    st["bpf_total"] = u32(st["bpf_total"] + pkt_len)
    st["bpf_reset"] = u32(st["bpf_reset"] + 1)
    if st["bpf_reset"] == 0:
        raise ValueError("bpf_reset wraps to 0: the reference divides by it")
    if isP:
        st["total_P_frame_q"] = s32(u32(st["total_P_frame_q"]) + st["rc_quant"])        # int += unsigned: unsigned sum, converted
        st["avg_P_frame_q"] = s32(u32(st["total_P_frame_q"]) // st["bpf_reset"])        # int / unsigned: unsigned division
        fps = u32(_fps_int(st, ov))                                                      # int division, into an unsigned
        if fps == 0:
            fps = 1
            L.add("fps_zero")
        need = (u32(st["bitrate"] << 5) // fps) >> 3
        t34 = u32(need * 3) // 4
        t78 = u32(need * 7) // 8
        under = pkt_len < t34
        went_over = pkt_len > t78
        if pkt_len == t34:
            L.add("P_eq_three_quarters")
        if pkt_len == t78:
            L.add("P_eq_seven_eighths")
        L.add("P_over" if went_over else "P_under" if under else "P_between")
        st["back_into_range"] = 1 if (st["last_P_frame_over"] and under) else 0
        if st["back_into_range"]:
            L.add("back_set")
        st["last_P_frame_over"] = 1 if went_over else 0
    else:
        st["last_P_frame_over"] = 0
        st["back_into_range"] = 0
        L.add("I_clears")
    st["bpf_avg"] = s32(st["bpf_total"] // st["bpf_reset"])
    if st["bpf_reset"] >= BPF_RESET:
        st["bpf_total"] = u32(st["bpf_avg"])
        st["total_P_frame_q"] = s32(u32(st["total_P_frame_q"]) // st["bpf_reset"])
        st["bpf_reset"] = 1
        L.add("wrap_P" if isP else "wrap_I")
    st.overflow = st.overflow or ov.hit
    return st, L


def seg_bits(v):
    """bits of dsv_bs_put_seg(v) (bs.c:147-157): the interleaved exp-Golomb code of |v| -- a zero and a data bit per bit below the
    leading one of |v| + 1, then the stop bit -- and a sign bit unless v is 0"""
    m = abs(v) + 1
    return 2 * (m.bit_length() - 1) + 1 + (1 if v else 0)


def packet_len(prefix_len, dc, total_bits):
    """bytes of a picture packet -> (len, labels): prefix_len bytes up to the quantiser field, the 11-bit quantiser (the planes start
    byte aligned: 2 bytes), then per plane the 32-bit length, SEG(dc), alignment, the 32-bit run count, the payload, the 0x55 byte"""
    L = set()
    n = prefix_len + 2
    for p in range(3):
        m = abs(dc[p]) + 1
        if dc[p] == 0:
            L.add("dc0")
        if dc[p] < 0:
            L.add("dc_negative")
        for k, name in ((15, "dc_1byte_max"), (16, "dc_2byte_min"), (255, "dc_2byte_max"), (256, "dc_3byte_min")):
            if m == k:
                L.add(name)
        L.add("bits_zero" if total_bits[p] == 0 else "bits_mult8" if total_bits[p] % 8 == 0 else "bits_not_mult8")
        n += 4 + (seg_bits(dc[p]) + 7) // 8 + 4 + u32((total_bits[p] + 7) >> 3) + 1
    return u32(n), L


# ---- what a frame quantiser determines in a picture's job record -------------------------------------------------------------------
def get_quant(q, isP, level):                                  # dsv_get_quant hzcc.c:77-92
    if isP:
        q = q * 3 // 2
    if level == 1:
        q = q * 2 // 3
    elif level == 2:
        q = q * 3 // 2
    return max(q, 16)


def lb2(n):                                                    # dsv_lb2 hzcc.c:437-447: the smallest l with 2^l >= n
    l = 0
    while (1 << l) < n:
        l += 1
    return l


def job_quant_tables(quant, isP):
    """-> (pairs[3][10] of (qp, qp_h), hqp[16]): the ten scan regions of each plane in scan order (the LL region, then levels 0..2 with
    three subbands each; hzcc.c:156-162,190-208: level 2 carries shifts), and the luma smoothing bounds by level (sbt.c:677-696; entry 0
    is unused by the reference and holds the LL value in the product's record)"""
    pairs = []
    for plane in range(3):
        q = min(quant, 512) if plane > 0 else quant            # fix_quant hzcc.c:50-57, CHROMA_LIMIT
        row = [(get_quant(q, isP, 0), 0)]
        for l in range(3):
            qp, qp_h = get_quant(q, isP, l), 0
            if l == 2:
                qp = lb2(qp)
                qp_h = clamp(qp - (1 if isP else 3), 1, 24)[0]  # DSV_QP_P / DSV_QP_I
            row += [(qp, qp_h)] * 3
        pairs.append(row)
    llq = get_quant(quant, isP, 0) // 2
    hqp = []
    for i in range(16):
        if i > 3 or i == 0:
            v = llq
        else:
            v = get_quant(quant, isP, 3 - i)
            if i == 1:
                v = clamp(lb2(v) - (1 if isP else 3), 1, 24)[0]
                v = (1 << v) >> 1
            v //= 2
        hqp.append(v)
    return pairs, hqp


def job_table_words(quant, isP):
    """the 76 words dsv1_rc_job_tables / dsvg_op_rc return: plane-major (qp, qp_h) pairs, then hqp[16]"""
    pairs, hqp = job_quant_tables(quant, isP)
    return [w for row in pairs for pr in row for w in pr] + hqp


_QUALITY_OF = {}


def state_for_quant(fq, isP=0):
    """a state from which pick(isP, not forced) returns exactly the frame quantiser fq (5..2047: every one has a quality that maps to
    it): bpf_avg == need makes the step 0, the bounds are wide open"""
    if not _QUALITY_OF:
        for q in range(MAXQ, -1, -1):
            _QUALITY_OF[MAXQ - (MAXQ - 5) * q // MAXQ] = q
    return make_state(rc_quant=_QUALITY_OF[fq], bitrate=240000, bpf_avg=1000, min_quality=0, max_quality=MAXQ, min_I_frame_quality=0,
                      avg_P_frame_q=0, bpf_reset=10, bpf_total=10000)


# ---- the generator shared by the host and the device tests -------------------------------------------------------------------------
TIER_EDGES = (PCT(60), PCT(70), PCT(75), 0, MAXQ, PCT(5), PCT(95))


def _near(r, c, w):
    return c + r.randint(-w, w)


def draw_case(r):
    """one random (state, isP, forced_intra, pkt_len) drawn so that every label has a probability of a few percent or more; never a
    state that divides by zero.  Overflow cases are possible (rare) and are the caller's to drop."""
    while True:
        st = make_state()
        u = r.random()
        if u < 0.12:
            st["fps_num"], st["fps_den"] = r.randint(0, 3), r.randint(97, 4000)                  # fps == 0
        elif u < 0.5:
            st["fps_num"], st["fps_den"] = r.choice(((30, 1), (25, 1), (30000, 1001), (24000, 1001), (60, 1), (15, 2)))
        else:
            st["fps_num"], st["fps_den"] = r.randint(1, 240), r.randint(1, 8)
        st["bitrate"] = r.choice((r.randint(2000, 100000), r.randint(100000, 60000000), r.randint(1 << 27, (1 << 32) - 1)))
        if u < 0.12 and r.random() < 0.7:
            st["bitrate"] = r.randint(2000, 250000)                                              # need = 4 * bitrate there
        try:
            need = needed_bpf(st)
        except ValueError:
            continue
        if need > (1 << 20):                                   # abs(bpf - need) << 9 would leave int32 for most of these
            continue
        st["rc_high_motion_nudge"] = 0 if r.random() < 0.12 else r.choice((1, 1, 1, 2, -1))
        u = r.random()
        st["max_q_step"] = (r.randint(-3, 0) if u < 0.06 else r.randint(2048, 6000) if u < 0.12 else r.randint(1, 40) if u < 0.8 else r.randint(1, MAXQ))
        u = r.random()
        if u < 0.52:
            st["min_quality"], st["max_quality"] = r.randint(0, 400), r.randint(1200, MAXQ)
        elif u < 0.60:
            st["min_quality"], st["max_quality"] = r.randint(800, MAXQ), r.randint(0, 799)       # inverted
        elif u < 0.76:
            st["min_quality"], st["max_quality"] = r.randint(0, 50), r.randint(0, PCT(5) + 20)   # ceiling minus 5 % negative
        elif u < 0.84:
            st["min_quality"], st["max_quality"] = r.randint(0, 400), r.randint(2048, 4000)      # final clamp
        else:
            st["min_quality"], st["max_quality"] = sorted((r.randint(0, MAXQ), r.randint(0, MAXQ)))
        st["min_I_frame_quality"] = r.choice((PCT(5), r.randint(0, MAXQ)))
        u = r.random()
        st["rc_quant"] = (_near(r, r.choice(TIER_EDGES), 3) if u < 0.35 else r.randint(0, MAXQ) if u < 0.95 else r.randint(MAXQ + 1, 5000))
        st["rc_quant"] = max(st["rc_quant"], 0)
        u = r.random()
        if u < 0.08:
            st["bpf_avg"] = 0
        elif u < 0.16:
            st["bpf_avg"] = need
        elif u < 0.7:
            st["bpf_avg"] = max(1, need + r.randint(-need // 8 - 2, need // 8 + 2))              # around need: small steps
        else:
            st["bpf_avg"] = r.randint(1, min(4 * need + 10, (1 << 22)))
        u = r.random()
        st["bpf_reset"] = (r.randint(252, 256) if u < 0.15 else r.randint(0, 251))
        st["bpf_total"] = u32(st["bpf_avg"] * st["bpf_reset"] + r.randint(0, max(st["bpf_reset"], 1)))
        st["avg_P_frame_q"] = r.choice((r.randint(0, MAXQ), _near(r, st["min_quality"] + PCT(4), 3), _near(r, st["max_quality"] + PCT(4), 3)))
        st["total_P_frame_q"] = st["avg_P_frame_q"] * max(st["bpf_reset"], 1) + r.randint(0, 200)
        if r.random() < 0.04:
            st["total_P_frame_q"] = -r.randint(1, 1 << 20)                                       # the division by bpf_reset is unsigned
        u = r.random()
        st["last_P_frame_over"], st["back_into_range"] = ((0, 0) if u < 0.4 else (1, 0) if u < 0.65 else (0, 1) if u < 0.9 else (1, 1))
        isP = 1 if r.random() < 0.6 else 0
        forced = 1 if (not isP and r.random() < 0.5) else 0
        if forced and r.random() < 0.6:
            st["rc_quant"] = _near(r, r.choice((PCT(60), PCT(70), PCT(75))), 30)                 # the forced-intra tiers' borders
        n2 = (u32(st["bitrate"] << 5) // max(1, u32(tdiv(st["fps_num"] << 5, st["fps_den"])))) >> 3
        t34, t78 = u32(n2 * 3) // 4, u32(n2 * 7) // 8
        u = r.random()
        pkt = (t34 if u < 0.08 else t78 if u < 0.16 else max(0, t34 - 1 - r.randint(0, 40)) if u < 0.4 else t78 + 1 + r.randint(0, 40) if u < 0.65
               else r.randint(t34, t78) if u < 0.8 else r.randint(0, 2 * n2 + 100))
        return st, isP, forced, u32(pkt)


def draw_packet(r):
    """(prefix_len, dc[3], total_bits[3]) around every byte border of the DC code and of the payload"""
    dc = []
    for _ in range(3):
        u = r.random()
        m = (r.choice((14, 15, 254, 255)) if u < 0.4 else 0 if u < 0.55 else r.randint(0, 70000))
        dc.append(-m if r.random() < 0.4 else m)
    bits = [r.choice((0, 8 * r.randint(1, 5000), r.randint(1, 400000))) for _ in range(3)]
    return r.randint(14, 4000), dc, bits


def rng(seed):
    return random.Random(seed)
