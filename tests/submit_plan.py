"""What an encoder session's submit decides, restated from the reference's side (dsv_encoder.c:538-554 scene change, 624-653 GOP
start / reference flags / forced intra, 665-708 which reconstructions exist and when the next GOP starts) and from the batch's
documented layout (include/dsv1_api.h, Submit plan).  Written on Python lists and dicts, frame by frame and stream by stream, with no
knowledge of csrc/host/dsv1_submit_plan.h: tests/test_submit_plan_host.py holds the library's query to it.

A source's state is a dict (next_fnum, prev_gop, gop, force_metadata, do_scd, prev_avg_luma, scene_change_delta); a stream's state a
dict (cur: the slot that holds its newest reconstruction or None, has_recon, border_skipped, recon_dropped).  Slots: a stream's pair
is {k, k + N}; chain mode has C + 1 pairs {2p, 2p + 1}."""
M32 = 0xFFFFFFFF
CLASSES = ("gop_by_count", "gop_by_force", "scene_cut", "forced_intra_pct", "dead_inside", "dead_at_end", "remedy", "extend",
           "chain_continued", "two_rounds", "run_merged", "run_split")


def gop_starts_at(src, fnum):
    """dsv_encoder.c:624: the addition wraps at 32 bits (prev_gop starts at -1)"""
    return bool(src["force_metadata"]) or ((src["prev_gop"] + src["gop"]) & M32) <= fnum


def encode_one_frame_decisions(src, mean_luma, seen):
    """dsv_encoder.c:624-652 for the source's next frame; returns the picture"""
    fnum = src["next_fnum"]
    src["next_fnum"] = (fnum + 1) & M32
    p = dict(fnum=fnum, gop_start=0, forced_intra=0, isP=0, n_intra=0)
    if gop_starts_at(src, fnum):
        seen["gop_by_force" if src["force_metadata"] else "gop_by_count"] += 1
        p["gop_start"] = 1
        src["prev_gop"] = fnum
        src["force_metadata"] = 0
    if src["gop"] == 0:
        p["is_ref"] = p["has_ref"] = 0
    else:
        p["is_ref"] = 1
        p["has_ref"] = 0 if p["gop_start"] else 1
        if src["do_scd"]:
            al = mean_luma()
            if abs(src["prev_avg_luma"] - al) > src["scene_change_delta"]:
                seen["scene_cut"] += p["has_ref"]
                p["has_ref"] = 0
                p["forced_intra"] = 1
            src["prev_avg_luma"] = al
    return p


def motion_est_decision(p, n_intra, nblk, thresh, seen):
    """dsv_encoder.c:238-253: too many intra blocks turn the picture intra"""
    if p["has_ref"]:
        p["n_intra"] = n_intra
        p["forced_intra"] = 0
        if n_intra * 100 // nblk > thresh:
            seen["forced_intra_pct"] += 1
            p["has_ref"] = 0
            p["forced_intra"] = 1
    p["isP"] = p["has_ref"]


def other_slot(pair, cur):
    return pair[1] if cur == pair[0] else pair[0]


def plan(g, srcs, streams, luma, n_intra, prev, seen):
    """one submit.  g: dict(S, R, F, nf, chains, gcount, par, npix_small, nblk, intra_pct_thresh, abr, serial, keep_all, nf_prev,
    carry=[pair, slot]); srcs / streams are updated, g["carry"] too.  prev: the pictures of the call before ({(k, t): pic}).
    Returns dict(pics {(k, t): pic}, pairs, ext, remedy_streams, remedy, jobs, calls, dropped); a job is a dict(pic=(k, t), ref, recon,
    out, hint, remedy).  None where chain mode refuses the call."""
    S, R, F, nf, C = g["S"], g["R"], g["F"], g["nf"], g["chains"]
    N, rows = S * R, 2 * g["F"] + 1
    pics, pairs, ext, rem_streams, remedy = {}, [], [], [], []
    for s in range(S):
        src = srcs[s]
        for t in range(nf):
            cur_slot = ((g["gcount"] + t) % rows) * S + s
            p = encode_one_frame_decisions(src, lambda: luma[cur_slot] // g["npix_small"], seen)
            p.update(cur_slot=cur_slot, ref_slot=((g["gcount"] + t + rows - 1) % rows) * S + s, out_slot=g["par"] * N * F + t * N + s * R)
            pics[(s * R, t)] = p
            if p["has_ref"]:
                pairs.append((p["cur_slot"], p["ref_slot"], s * R * F + t))
        first = pics[(s * R, 0)]
        for k in range(s * R, s * R + R):
            # what the call before promised on the strength of "the next picture starts a GOP" and the caller then broke by renumbering
            if first["has_ref"] and streams[k]["border_skipped"]:
                ext.append(g["carry"][1] if C else streams[k]["cur"])
                seen["extend"] += 1
            if first["has_ref"] and streams[k]["recon_dropped"]:
                rem_streams.append(k)
            streams[k]["border_skipped"] = streams[k]["recon_dropped"] = 0
    for i, k in enumerate(rem_streams):
        pp = prev[(k, g["nf_prev"] - 1)]
        st = streams[k]
        new = other_slot((k, k + N), st["cur"])
        remedy.append(dict(pic=(k, g["nf_prev"] - 1), ref=st["cur"] if pp["isP"] else -1, recon=new, out=g["par"] * N * F + i, hint=0, remedy=1))
        st["cur"], st["has_recon"] = new, 1
        seen["remedy"] += 1
    for s in range(S):
        for t in range(nf):
            lead = pics[(s * R, t)]
            motion_est_decision(lead, n_intra[s * R * F + t], g["nblk"], g["intra_pct_thresh"], seen)
            for r in range(1, R):
                pics[(s * R + r, t)] = dict(lead, out_slot=lead["out_slot"] + r)
    next_gop = [gop_starts_at(srcs[k // R], srcs[k // R]["next_fnum"]) for k in range(N)]
    jobs, calls, dropped = [], [], 0
    if not C:
        by_step = [[None] * N for _ in range(nf)]
        for k in range(N):                                  # a stream at a time, in coding order
            st = streams[k]
            if st["cur"] is None:
                st["cur"] = k
            for t in range(nf):
                p = pics[(k, t)]
                last = t + 1 == nf
                # dsv_encoder.c:665-674 builds a reconstruction for every reference picture; only the next picture of the stream ever reads it
                if last:
                    read = not (next_gop[k] and not g["abr"])
                    known = next_gop[k]
                else:
                    read = bool(pics[(k, t + 1)]["isP"])
                    known = True
                if g["serial"] or g["keep_all"]:
                    read = True
                if g["serial"]:
                    known = False
                j = dict(pic=(k, t), ref=st["cur"] if p["isP"] else -1, recon=-1, out=p["out_slot"], hint=int(known), remedy=0)
                if p["is_ref"] and read:
                    j["recon"] = st["cur"] = other_slot((k, k + N), st["cur"])
                    st["has_recon"] = 1
                elif p["is_ref"]:
                    dropped += 1
                    seen["dead_at_end" if last else "dead_inside"] += 1
                if last:
                    st["recon_dropped"] = int(bool(p["is_ref"] and not read))
                    st["border_skipped"] = int(j["hint"] and j["recon"] >= 0)
                by_step[t][k] = j
        jobs = [j for step in by_step for j in step]
        calls = [dict(nsteps=1, njobs=N, first=t * N) for t in range(nf)] if g["serial"] else [dict(nsteps=nf, njobs=N, first=0)]
    else:
        st = streams[0]
        chains = []
        for t in range(nf):
            if t == 0 or not pics[(0, t)]["isP"]:
                chains.append([])
            chains[-1].append(t)
        cont = bool(pics[(0, 0)]["isP"])
        if cont and g["carry"][1] < 0:
            return None
        seen["chain_continued"] += cont
        seen["two_rounds"] += len(chains) > C
        out = g["par"] * F
        state = {}                                           # chain -> [pair, newest slot]
        for r0 in range(0, len(chains), C):
            rnd = list(range(r0, min(r0 + C, len(chains))))
            free = [p for p in range(C + 1) if not (r0 == 0 and cont and p == g["carry"][0])]
            for c in rnd:
                state[c] = [g["carry"][0], g["carry"][1]] if (c == 0 and cont) else [free.pop(0), -1]
            depth = max(len(chains[c]) for c in rnd)
            live = [[c for c in rnd if len(chains[c]) > k] for k in range(depth)]
            k = 0
            while k < depth:
                k2 = k + 1
                while k2 < depth and len(live[k2]) == len(live[k]):
                    k2 += 1
                seen["run_merged"] += k2 - k > 1
                seen["run_split"] += k2 < depth
                calls.append(dict(nsteps=k2 - k, njobs=len(live[k]), first=len(jobs)))
                for kk in range(k, k2):
                    for c in live[kk]:
                        t = chains[c][kk]
                        p = pics[(0, t)]
                        end = kk + 1 == len(chains[c])
                        pair = (2 * state[c][0], 2 * state[c][0] + 1)
                        j = dict(pic=(0, t), ref=state[c][1] if p["isP"] else -1, recon=-1, out=out, hint=0, remedy=0)
                        p["out_slot"] = out
                        out += 1
                        if p["is_ref"] and end and t + 1 < nf and not g["keep_all"]:
                            dropped += 1
                            seen["dead_inside"] += 1
                        elif p["is_ref"]:
                            j["recon"] = state[c][1] = other_slot(pair, state[c][1])
                        # the reader of this reconstruction: the chain's next picture if it is coded by this very call; none if the
                        # stream goes on with an I picture; unknown otherwise
                        if not end:
                            j["hint"] = int(kk + 1 < k2)
                        elif t + 1 < nf:
                            j["hint"] = 1
                        else:
                            j["hint"] = int(next_gop[0])
                        if t + 1 == nf:
                            st["border_skipped"] = int(j["hint"] and j["recon"] >= 0)
                        jobs.append(j)
                k = k2
        if pics[(0, nf - 1)]["is_ref"]:
            g["carry"] = list(state[len(chains) - 1])
            st["has_recon"] = 1
    return dict(pics=pics, pairs=pairs, ext=ext, remedy_streams=rem_streams, remedy=remedy, jobs=jobs, calls=calls, dropped=dropped,
                next_gop=next_gop)
