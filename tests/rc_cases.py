"""Built inputs for the rate-control tests: the launches of tests/test_gpu_rc_paths.py's operator part (one launch_rc each, expected
results from tests/rc_model.py), and RC_SEEDS, the seeded sessions of tests/test_rc_ref.py and of the same GPU file."""
import rc_model as M

POISON = 0x5A5A5A5A

# ---- operator launches ---------------------------------------------------------------------------------------------------------------
OP_COUNTS = (1, 63, 64, 65, 130)
OP_D0 = (0, 37)
OP_LAUNCHES = [(count, d0, mode) for count in OP_COUNTS for d0 in OP_D0 for mode in (0, 1)]


def _packet_for(r, pkt):
    """(prefix_len, dc[3], total_bits[3]) of a packet of pkt bytes where one that short exists, else of the shortest one"""
    _, dc, _ = M.draw_packet(r)
    over = 2 + sum(9 + (M.seg_bits(v) + 7) // 8 for v in dc)
    room = max(0, pkt - over)
    prefix = min(room, r.randint(14, 4000))
    room -= prefix
    a = r.randint(0, room)
    b = r.randint(0, room - a)
    nb = [a, b, room - a - b]
    r.shuffle(nb)
    bits = [0 if n == 0 else 8 * n - (r.randint(0, 7) if r.random() < 0.6 else 0) for n in nb]
    return prefix, dc, bits


class OpLaunch:
    """one launch_rc over n job records and nslots states.  Inputs: jobs (dicts of the dsvg_op_rc_job fields), states (rc_model
    states by slot).  Expected, from the model: want_states (by slot), want_quant / want_tables / want_rc by job, labels."""

    def __init__(self, seed, count, d0, mode):
        r = M.rng(seed)
        tail = count + r.randint(3, 9)                         # jobs behind the range: the next frame step's
        n = d0 + count + tail
        nslots = n + n // 3 + 3                                # holes
        slots = list(range(nslots))
        r.shuffle(slots)
        self.n, self.nslots, self.d0, self.count, self.mode = n, nslots, d0, count, mode
        self.labels = set()
        outside = [j for j in range(n) if not d0 <= j < d0 + count]
        r.shuffle(outside)
        states = [None] * nslots
        jobs = []
        for j in range(n):
            st, isP, fi, pkt = M.draw_case(r)
            prefix, dc, bits = _packet_for(r, pkt)
            slot = -1 if r.random() < 0.1 else slots[j]
            jobs.append(dict(isP=isP, forced_intra=fi, prefix_len=prefix, slot=slot, next=-1, quant=r.randint(5, M.MAXQ), dc=dc, total_bits=bits))
            states[slots[j]] = st                              # a skipped job's state is there all the same, and must stay
        for s in range(nslots):
            if states[s] is None:
                states[s] = M.draw_case(r)[0]
        self.want_states = [s.copy() for s in states]
        self.want_quant = [jb["quant"] for jb in jobs]
        self.want_tables = [[POISON] * 76 for _ in range(n)]
        self.want_rc = [[POISON] * 3 for _ in range(n)]
        for j in range(d0, d0 + count):
            jb = jobs[j]
            if mode == 1 and r.random() < 0.8 and outside:
                jb["next"] = outside.pop()                     # no two jobs of a launch share a next
            if jb["slot"] < 0:
                continue
            while True:                                        # a case the model marks as overflow is fed to nothing: draw that job's state again
                try:
                    res = self._model(jobs, j, states[jb["slot"]])
                except ValueError:
                    res = None
                if res is not None and not res[0].overflow:
                    break
                states[jb["slot"]] = M.draw_case(r)[0]
                self.want_states[jb["slot"]] = states[jb["slot"]].copy()
            st, labels, writes = res
            self.want_states[jb["slot"]] = st
            self.labels |= labels
            for k, v in writes.items():
                getattr(self, k)[v[0]] = v[1]
        self.jobs, self.states = jobs, states
        self.check_inputs()

    def _model(self, jobs, j, st):
        jb = jobs[j]
        writes = {}
        if self.mode == 0:
            fq, st, l = M.pick(st, jb["isP"], jb["forced_intra"])
            labels = {"pick." + x for x in l}
            writes["want_quant"] = (j, fq)
            writes["want_tables"] = (j, M.job_table_words(fq, jb["isP"]))
            return st, labels, writes
        ln, l = M.packet_len(jb["prefix_len"], jb["dc"], jb["total_bits"])
        labels = {"packet." + x for x in l}
        writes["want_rc"] = (j, [jb["quant"], ln, 0])
        st, l = M.after(st, jb["isP"], ln)
        labels |= {"after." + x for x in l}
        if jb["next"] >= 0:
            nx = jobs[jb["next"]]
            fq, st, l = M.pick(st, nx["isP"], nx["forced_intra"])
            labels |= {"pick." + x for x in l}
            writes["want_quant"] = (jb["next"], fq)
            writes["want_tables"] = (jb["next"], M.job_table_words(fq, nx["isP"]))
        return st, labels, writes

    def check_inputs(self):
        """what k_rc's one thread per job relies on: no two launched jobs share a state or a next, and a next lies outside the
        launched range (it is a later frame step's job: a launched job's own record is being read)"""
        live = [jb for jb in self.jobs[self.d0:self.d0 + self.count] if jb["slot"] >= 0]
        sl = [jb["slot"] for jb in live]
        assert len(set(sl)) == len(sl) and all(0 <= s < self.nslots for s in sl)
        if self.mode == 1:
            nx = [jb["next"] for jb in live if jb["next"] >= 0]
            assert len(set(nx)) == len(nx)
            assert all(0 <= t < self.n and not self.d0 <= t < self.d0 + self.count for t in nx)


def op_launches():
    return [OpLaunch(0xAB0 + 17 * i, c, d0, mode) for i, (c, d0, mode) in enumerate(OP_LAUNCHES)]


class QuantDomainLaunch(OpLaunch):
    """mode 0, one job per frame quantiser 5..2047 and picture type: 4086 jobs whose states make pick return exactly that value"""

    def __init__(self):
        want = [(fq, isP) for isP in (0, 1) for fq in range(5, M.MAXQ + 1)]
        n = len(want)
        self.n = self.nslots = self.count = n
        self.d0, self.mode = 0, 0
        self.jobs = [dict(isP=isP, forced_intra=0, prefix_len=0, slot=j, next=-1, quant=POISON, dc=[0, 0, 0], total_bits=[0, 0, 0])
                     for j, (fq, isP) in enumerate(want)]
        self.states = [M.state_for_quant(fq, isP) for fq, isP in want]
        res = [M.pick(st, isP, 0) for st, (fq, isP) in zip(self.states, want)]
        assert [x[0] for x in res] == [fq for fq, _ in want]
        self.want_states = [x[1] for x in res]
        self.want_quant = [fq for fq, _ in want]
        self.want_tables = [M.job_table_words(fq, isP) for fq, isP in want]
        self.want_rc = [[POISON] * 3 for _ in range(n)]
        self.labels = set()
        self.check_inputs()


# ---- seeded sessions -----------------------------------------------------------------------------------------------------------------
# The encoder struct's rate-control state is public and has the reference's layout, so a session can be put a few pictures before
# any branch: RC_SEEDS codes 176x144 4:2:0 clips of 8 to 14 frames through the reference library, the oracle, the model and (on the
# GPU) the product's three session paths.  Scene-cut detection is off in every case: a forced-intra picture is then exactly an intra
# picture that is not a GOP start (motion_est's intra-block rule, dsv_encoder.c:248-252), which the model's replay reads off the packets.
# F, calls: how the GPU sessions cut the clip into calls; a case's `changes` fall on call borders (a batch takes them between submits).
# Bitrates come from the packet sizes the REFERENCE library produces for the clip (noted on each case), never from the product.
W, H, FRAMES_MAX = 176, 144, 14
Q = M.PCT


def _case(name, labels, frames, style, clip, gop=12, qp=60, ipct=50, bitrate=64597, par=None, seed=None, changes=None, F=None, calls=1):
    par = dict(par or {})
    par["bitrate"] = bitrate
    return dict(name=name, labels=set(labels), frames=frames, style=style, clip=clip, cli=dict(qp=qp, gop=gop, rc_mode_cli=0, scd=0, ipct=ipct),
                par=par, seed=dict(seed or {}), changes=changes or {}, F=F or frames, calls=calls)


def cfg_fields(case):
    """(public parameter fields, (fps_num, fps_den)) a case sets on top of the CLI's defaults"""
    par = dict(case["par"])
    fps = (par.pop("fps_num", 30), par.pop("fps_den", 1))
    return par, fps


def initial_state(case):
    """the model's state before the first picture: the CLI's defaults (dsv_main.c:423-489), dsv_enc_start, the case's parameters, its seed"""
    quality = min(M.MAXQ * case["cli"]["qp"] // 100 * 3 // 2, M.MAXQ)
    par, fps = cfg_fields(case)
    st = M.make_state(rc_quant=quality, avg_P_frame_q=quality * 4 // 5, max_quality=M.MAXQ, fps_num=fps[0], fps_den=fps[1])
    st.update(par)
    st.update(case["seed"])
    return st


def replay(case, packets):
    """the model over a coded stream's picture packets (bytes each) -> ([state words after each picture], labels, final state)"""
    st = initial_state(case)
    gop = case["cli"]["gop"]
    out, labels = [], set()
    for t, p in enumerate(packets):
        st.update(case["changes"].get(t, {}))
        isP = p[5] & 1
        forced = 1 if (gop and not isP and t % gop) else 0
        _, st, l1 = M.pick(st, isP, forced)
        st, l2 = M.after(st, isP, len(p))
        assert not st.overflow, "%s: picture %d overflows" % (case["name"], t)
        labels |= {"pick." + x for x in l1} | {"after." + x for x in l2}
        out.append(tuple(M.u32(st[f]) for f in M.STATE_FIELDS))
    return out, labels, st


def _mid_stream(reset, avg, q):
    """a consistent state `reset` pictures into an averaging window: totals that give these averages"""
    return dict(bpf_reset=reset, bpf_total=reset * avg, bpf_avg=avg, total_P_frame_q=reset * q, avg_P_frame_q=q, rc_quant=q + 80)


_PIN = dict(min_quality=Q(70), max_quality=Q(70), min_I_frame_quality=Q(70))       # every picture at quality 70 %: sizes independent of the bitrate

RC_SEEDS = [
    # the 256-picture renormalisation on a P picture mid-stream (the third picture).  Reference: I1831 P149 P186 P206 P193 P204 P197 P197;
    # the CLI's own bitrate for this geometry (64597: 269 bytes per frame), the window's average seeded at 600
    _case("wrap_P", ["wrap_P", "P_under", "P_between"], 8, 0, 0x5EED0, seed=_mid_stream(253, 600, 1400), F=4, calls=2),
    # the same on an intra-only stream; the seeded back_into_range nudges the first I picture up.  Reference: I pictures of 1650..2031
    # bytes; 1200000 bit/s = 5000 bytes per frame = the seeded average
    _case("wrap_I", ["wrap_I", "nudge_up_I", "I_clears"], 8, 0, 0x5EED1, gop=0, bitrate=1200000, seed=dict(_mid_stream(253, 5000, 1400), back_into_range=1)),
    # the counter reaches 256 on the sixth picture: the last one of a 6-frame call while the next call is enqueued (GPU, pipelined).
    # Reference: I1889 P150 P174 P198 P192 P190 P194 I1911 (forced) P195 P202 P224 P191
    _case("wrap_last_of_call", ["wrap_P"], 12, 3, 0x5EED2, seed=_mid_stream(250, 600, 1400), F=6, calls=2),
    # P pictures over the budget, then a bitrate change (between two calls of 5) brings one under.  Reference: I8573 P334 P238 P187 P175 |
    # P226 ...: 30000 bit/s = 125 bytes per frame (7/8: 109) puts every P over; 400000 from the sixth picture = 1666 (3/4: 1250) puts it under
    _case("over_then_under", ["nudge_down", "back_set", "nudge_up_P", "cap16", "P_over", "P_under"], 10, 0, 0x5EED3, bitrate=30000,
          seed=dict(rc_quant=1900), changes={5: dict(bitrate=400000)}, F=5, calls=2),
    # a P picture over the budget right before a GOP start (picture 12).  Reference P pictures 276..746 bytes; 40000 bit/s = 166 per frame
    _case("gop_start_after_over", ["I_ignores_over", "floor_hit"], 14, 5, 0x5EED4, bitrate=40000, F=7, calls=2),
    _case("nudge_off", ["nudge_off"], 8, 0, 0x5EED5, par=dict(rc_high_motion_nudge=0), seed=dict(last_P_frame_over=1, back_into_range=1), F=4, calls=2),
    _case("step_lo", ["step_lo"], 8, 0, 0x5EED6, par=dict(max_q_step=0), F=4, calls=2),
    _case("step_hi", ["step_hi"], 8, 0, 0x5EED7, par=dict(max_q_step=5000), F=4, calls=2),
    _case("bounds_inverted", ["bounds_inverted", "p_floor_min", "ceiling_hit"], 8, 0, 0x5EED8, par=dict(min_quality=Q(70), max_quality=Q(40)), F=4, calls=2),
    # forced-intra pictures (clip style 1 with a 20 % intra-block threshold) under a ceiling below 5 %: the forced-intra clamp's upper
    # bound is negative
    _case("ceiling_negative", ["fi_ceiling_negative", "i_floor_hit", "p_floor_max", "quant_ends"], 8, 1, 0x5EED9, ipct=20,
          par=dict(max_quality=Q(3), min_quality=0, min_I_frame_quality=0)),
    # 1/64 frames per second: fps == 0 becomes 1; 300 bit/s = 1200 bytes per frame there
    _case("fps_zero", ["fps_zero"], 8, 0, 0x5EEDA, par=dict(fps_num=1, fps_den=64), bitrate=300),
    # the forced-intra tiers from below 60 % upwards.  Reference: I pictures of 987..2007 bytes; 600000 bit/s = 2500 per frame keeps the
    # stream under the budget, so the quality climbs through the tiers
    _case("fi_tiers", ["fi_lt60", "fi_lt75", "fi_none"], 8, 1, 0x5EEDB, ipct=20, bitrate=600000,
          seed=dict(rc_quant=Q(60) - 60, bpf_avg=1000, bpf_reset=4, bpf_total=4000)),
    _case("fi_ceiling", ["fi_lt70", "fi_ceiling"], 8, 1, 0x5EEDD, ipct=20, bitrate=600000, par=dict(max_quality=Q(72)),
          seed=dict(rc_quant=Q(62), bpf_avg=1000, bpf_reset=4, bpf_total=4000)),
    # the second picture is forced intra at exactly 70 % (1432 = the seed + two capped steps of 10): the middle tier's border is exclusive
    _case("fi_at_70_percent", ["fi_lt75", "cap"], 8, 1, 0x5EEDF, ipct=20, bitrate=600000,
          seed=dict(rc_quant=Q(70) - 20, bpf_avg=1000, bpf_reset=4, bpf_total=4000)),
    # a ceiling above 2047 (the field is the caller's): the last clamp is the one that holds
    _case("final_clamp", ["final_clamp", "quant_ends"], 8, 0, 0x5EEDC, bitrate=3000000, par=dict(max_quality=3000), seed=dict(rc_quant=2040), F=4, calls=2),
    # packet sizes exactly on the two thresholds.  Every picture is coded at 70 % whatever the bitrate; the reference's P pictures are
    # 160 173 198 182 212 181 200 bytes.  55440 bit/s = 231 per frame, 231 * 3 / 4 = 173 = the third picture; 49920 from the fifth
    # picture = 208 per frame, 208 * 7 / 8 = 182 = the fifth picture
    _case("thresholds", ["P_eq_three_quarters", "P_eq_seven_eighths", "P_between"], 8, 0, 0x5EEDE, par=_PIN, bitrate=55440, changes={4: dict(bitrate=49920)}, F=4, calls=2),
]
RC_SEED_NAMES = [c["name"] for c in RC_SEEDS]

# pick / after labels the table does not have to reach (tests/test_rc_host.py and the operator launches do): none -- every branch can
# be put within a few pictures of a seeded session.  {label: why a real session cannot get there}
SESSION_UNREACHABLE = {}
