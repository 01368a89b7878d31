#!/usr/bin/env python3
"""What a quality ladder (dsv1_ladder_open, Python Ladder) saves on the headline shape: 1920x1080 4:2:0, GOP 12, --gops closed GOPs per
step, steps pipelined as bench.py runs them (stage(i+1); submit(i+1); collect(i)).  For every rung count R of --rungs, with the clip held
in HBM (DSV1_CLIP_HELD) and in pinned host memory (one upload per step inside the step), it times
    ladder:   ONE Ladder of R rungs (qp RUNG_QP[:R]): one upload, one load + pyramid, one motion search per step for all R rungs;
    separate: R plain Batches, one per rung, run back to back (each opened, timed over the same steps, closed: the sum of their times).
Both forms start from a fresh open and code the same submits, so the last timed step of every rung must hash the same in both.  Prints
one JSON line per (input, R, form) -- rung-pixel rate (R x pixels per step / time), ms per step, the device-side breakdown of the
pipeline's streams (Batch.breakdown_stop: load_pyramid, motion_search, table_uploads, coding_stream0/1 ...) -- and a summary line:
    python tools/ladder_cost.py [--gops 320] [--steps 4] [--rungs 1,2,3,4] [--inputs held,pinned]
Like bench.py, the process first moves to the host cores the link is best from (shard.pin_single_rank_measured); --no-pin: it stays."""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _cabi as A  # noqa: E402

W, H, FMT, GOP = 1920, 1080, A.SUBSAMP_420, 12
RUNG_QP = [85, 95, 70, 50]          # rung 0 is bench.py's headline quantiser


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=320)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rungs", default="1,2,3,4")
    ap.add_argument("--inputs", default="held,pinned")
    ap.add_argument("--no-pin", action="store_true")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic GOP clips (bench.py's default and seeds)")
    args = ap.parse_args()
    rung_counts = [int(x) for x in args.rungs.split(",")]
    inputs = [x.strip() for x in args.inputs.split(",")]
    assert all(1 <= r <= len(RUNG_QP) for r in rung_counts) and all(i in ("held", "pinned") for i in inputs)
    placement = None
    if not args.no_pin:
        shard = importlib.import_module("digital-subband-video-1_amd.shard")
        _, node, _ = shard.pin_single_rank_measured(0)        # before anything touches the GPU
        placement = "numa node %s" % node if node is not None else "unpinned"
    pkg = importlib.import_module("digital-subband-video-1_amd")
    if pkg.lib().dsvg_device_count() < 1:
        raise RuntimeError("no HIP device")
    fb = A.frame_bytes(W, H, FMT)
    nd = max(1, min(args.distinct, args.gops))
    distinct = [A.gen_clip(W, H, FMT, 0x10800003 + g, GOP, style=0) for g in range(nd)]
    pix_step = args.gops * GOP * W * H

    def cfg(qp):
        return pkg.make_encoder_cfg(W, H, FMT, qp=qp, gop=GOP, rc_mode_cli=1)

    def timed(b, inp):
        """fill + --steps timed steps -> (seconds, breakdown, last step's outputs as bytes)"""
        shape = (args.gops, GOP, fb)
        if inp == "held":
            host = np.empty(shape, dtype=np.uint8)
            for s in range(args.gops):
                host[s] = distinct[s % nd]
            src = b.upload(host)
            del host
        else:
            src = b.pinned(shape)
            for s in range(args.gops):
                src[s] = distinct[s % nd]
        ondev = inp == "held"
        b.submit(src, on_device=ondev, held=True)           # fill the pipeline
        b.sync()
        b.breakdown_start()
        t0 = time.perf_counter()
        if not ondev:
            b.stage(src)
        for i in range(args.steps):
            if not ondev and i + 1 < args.steps:
                b.stage(src)
            b.submit(src, on_device=ondev, held=True)
            outs = b.collect(copy=False)
        b.sync()
        dt = time.perf_counter() - t0
        bd = b.breakdown_stop(args.steps)
        last = [bytes(o) for o in outs]
        del outs
        b.collect(copy=False)                                # drain
        return dt, bd, last

    def rung_hashes(streams, R, index):
        return [hashlib.sha256(b"".join(streams[index(s, r)] for s in range(args.gops))).hexdigest() for r in range(R)]

    recs, summ = [], {"shape": "%dx%d 4:2:0 GOP %d qp %s, %d GOPs per step" % (W, H, GOP, RUNG_QP, args.gops), "steps": args.steps,
                      "placement": placement}
    for inp in inputs:
        for R in rung_counts:
            res = {}
            try:
                b = pkg.Ladder([cfg(q) for q in RUNG_QP[:R]], args.gops, GOP)
                try:
                    dt, bd, last = timed(b, inp)
                finally:
                    b.close()
                res["ladder"] = (dt, [bd], rung_hashes(last, R, lambda s, r: s * R + r))
                dts, bds, hs = 0.0, [], []
                for r in range(R):
                    b = pkg.Batch(cfg(RUNG_QP[r]), args.gops, GOP)
                    try:
                        dt, bd, last = timed(b, inp)
                    finally:
                        b.close()
                    dts += dt
                    bds.append(bd)
                    hs += rung_hashes(last, 1, lambda s, _r: s)
                res["separate"] = (dts, bds, hs)
            except RuntimeError as e:                       # (device memory for the largest ladders: reported, not hidden)
                rec = {"input": inp, "rungs": R, "error": str(e)}
                print(json.dumps(rec), flush=True)
                recs.append(rec)
                continue
            for form in ("ladder", "separate"):
                dt, bds, hs = res[form]
                dev = {k: round(sum(bd["device_ms_per_batch"][k] for bd in bds), 3) for k in
                       ("clip_upload", "load_pyramid", "motion_search", "table_uploads", "coding_stream0", "coding_stream1",
                        "fetch_gather_copy", "coding_overlapped_by_load_or_search")}
                rec = {"input": inp, "rungs": R, "form": form, "ms_per_step": round(1e3 * dt / args.steps, 3),
                       "rung_gpix_s": round(R * pix_step * args.steps / dt / 1e9, 2), "device_ms_per_step": dev,
                       "host_ms_per_step": {k: round(sum(bd["host_ms_per_batch"][k] for bd in bds), 3) for k in bds[0]["host_ms_per_batch"]},
                       "sha256_last_step_per_rung": hs}
                print(json.dumps(rec), flush=True)
                recs.append(rec)
            lad, sep = recs[-2], recs[-1]
            key = "%s_%d" % (inp, R)
            summ["ladder_over_separate_" + key] = round(lad["rung_gpix_s"] / sep["rung_gpix_s"], 3)
            summ["streams_equal_" + key] = lad["sha256_last_step_per_rung"] == sep["sha256_last_step_per_rung"]
    print(json.dumps({"summary": summ}), flush=True)
    if not all(v for k, v in summ.items() if k.startswith("streams_equal_")):
        sys.exit("a ladder's streams differ from the separate batches'")


if __name__ == "__main__":
    main()
