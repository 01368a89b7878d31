"""A packet fetch restated from its documented rules ("Packet fetch"; include/dsvg.h, dsvg_fetch_plan), not from
csrc/dsvg_fetch_plan.h: what dsvg_fetch_pictures_cb decides for a list of out slots, before and after the plane sizes are known.

  refusals    nchunks < 1, align < 1, n < 1 or n above the context's out slots: "bad fetch_pictures arguments"; a slot outside the
              context: "out slot out of range" (both -2); an overflowed plane, the first in picture-then-plane order:
              "packed plane P of out slot O exceeds CAP bytes" (-4)
  few         at most 4 pictures, no callback, the switch unset, every slot coded by the newest call (event (ncalls - 1) mod ring) or
              never, and no slot known to hold an I picture (a slot the P table does not reach counts as P)
  wait        the events of the slots, each once, in first-appearance order; in the fetch stream on the few path, on the host otherwise
  few copies  the pair grows to 4 * 3 * 65536 + 64; picture i plane p: min(65536, cap[p]) bytes from slot * per_job + off[p] to
              (3 i + p) * 65536; it delivers if every plane's bytes are within min(65536, cap[p]), else the general path runs
  general     summaries of slots min .. max; payloads in picture-then-plane order, each starting where the last ended rounded up to 16;
              the pair grows to total + 64; pieces: none asked without a callback; at most n // align; piece j of k ends at
              (n // align) * (j + 1) // k * align pictures, the last at n"""
ERR_ARG, ERR_OVERFLOW = -2, -4
K = 65536


class Refused(Exception):
    def __init__(self, rc, text):
        super().__init__(text)
        self.rc, self.text = rc, text


def bits_geo(cw, ch, cw2, ch2):
    """(bytes per job, plane offsets, plane capacities) of a job's packed bits as a context lays them out for coefficient planes of
    cw x ch (luma) and cw2 x ch2 (chroma): 16 bits per coefficient rounded up to 256, 256 bytes between planes"""
    cap = [(a * b * 2 + 255) & ~255 for a, b in ((cw, ch), (cw2, ch2), (cw2, ch2))]
    off = [0, cap[0] + 256, cap[0] + cap[1] + 512]
    return off[2] + cap[2] + 256, off, cap


def nbytes(bits):
    return (bits + 7) // 8


def plan(ctx_out_slots, out_slots, slot_ev, slot_isP, nring, ncalls, has_cb, no_fast, per_job, off, cap, total_bits, overflow, nchunks, align):
    n = len(out_slots)
    if nchunks < 1 or align < 1 or n < 1 or n > ctx_out_slots:
        raise Refused(ERR_ARG, "bad fetch_pictures arguments")
    if any(o < 0 or o >= ctx_out_slots for o in out_slots):
        raise Refused(ERR_ARG, "out slot out of range")
    d = {}
    newest = (ncalls - 1) % nring if ncalls > 0 else None
    few = n <= 4 and not has_cb and not no_fast
    few = few and all(slot_ev[o] < 0 or slot_ev[o] == newest for o in out_slots)
    few = few and all(o >= len(slot_isP) or slot_isP[o] for o in out_slots)
    d["few"] = d["stream_wait"] = int(few)
    d["wait"] = list(dict.fromkeys(slot_ev[o] for o in out_slots if slot_ev[o] >= 0))
    d["lo"], d["hi"] = min(out_slots), max(out_slots)
    d["grow_few"] = 4 * 3 * K + 64 if few else 0
    d["copies"] = [[(o * per_job + off[p], (3 * i + p) * K, min(K, cap[p])) for p in range(3)] for i, o in enumerate(out_slots)] if few else []
    for i, o in enumerate(out_slots):
        for p in range(3):
            if overflow[i][p]:
                e = Refused(ERR_OVERFLOW, "packed plane %d of out slot %d exceeds %d bytes" % (p, o, cap[p]))
                e.grow_few = d["grow_few"]
                raise e
    nb = [[nbytes(total_bits[i][p]) for p in range(3)] for i in range(n)]
    d["nbytes"] = nb
    d["fits"] = int(few and all(nb[i][p] <= min(K, cap[p]) for i in range(n) for p in range(3)))
    d["general"] = int(not d["fits"])
    if d["fits"]:
        d["pay"] = [[(3 * i + p) * K for p in range(3)] for i in range(n)]
        d.update(rows=[], total=0, grow=0, nchunks=0, pieces=[])
        return d
    total, rows = 0, []
    for i, o in enumerate(out_slots):
        rows.append([])
        for p in range(3):
            rows[-1].append((o * per_job + off[p], total, nb[i][p]))
            total += -(-nb[i][p] // 16) * 16
    d["rows"], d["total"], d["grow"] = rows, total, total + 64
    d["pay"] = [[r[1] for r in pic] for pic in rows]
    k = max(1, min(nchunks if has_cb else 1, n // align))
    ends = [n if j + 1 == k else (n // align) * (j + 1) // k * align for j in range(k)]
    start = lambda i: rows[i][0][1] if i < n else total
    d["nchunks"] = k
    d["pieces"] = [(a, b, start(a), start(b)) for a, b in zip([0] + ends[:-1], ends)]
    return d
