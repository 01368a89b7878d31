#!/usr/bin/env python3
"""bench.py -- encoded Mpixels/s of the MI355X-native DSV1 hot path, 1080p 4:2:0 GOP=12 (BASELINE.json).

A "step" = one pass of the whole per-frame hot path (pad/pyramid, HME, BMC, forward SBT, HZCC
quantise+pack, inverse SBT, reconstruction) PLUS the host session layer (side info, packet framing)
over one batch of synthetic input: --gops closed GOPs x 12 frames of 1920x1080 4:2:0, raw frames
already resident in HBM when the timed region starts; the output of a step is the finished .dsv bytes
of every GOP.  GOPs are independent (closed, CRF) so N GPUs shard them with no collective ("weak").

One JSON line on rank 0, see the keys at the bottom.  A plain run does what that line's headline needs and no more: it
sets up, warms up, times the steps, writes --dump-outputs and prints the line.  Everything else the benchmark measures or
checks runs with --full, after the headline: the CPU baseline (the REAL reference encoder, oracle/_ref where it was built,
otherwise our scalar port in oracle/, single thread, on a bounded sample of the same clips -- only a reported number), the
bit-exact checks of the timed output against the reference, the per-kernel roofline, the NUMA placement measured over
the link, the host-fed figure, the other shapes and config 4's sharded leg.
"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, FMT, GOP = 1920, 1080, 0x5, 12
QP = 85
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# VALU issue roof, MEASURED on this chip (tools/ubench/valu_rates.hip, kept in profiles/r03_valu_rates.txt; 8 waves per SIMD,
# chip-wide G wave64-instructions/s): the integer / byte / packed-16 forms these kernels are made of (v_sad_u8 516, v_perm_b32
# 526, v_alignbyte_b32 539, v_dot4_u32_u8 528, v_mul_lo_u32 536, v_pk_add_i16 534, v_pk_max_i16 530, v_med3_i32 534, v_bfe_u32 545,
# v_lshl_add_u32 518, v_cndmask_b32_e64 529) issue once per ~4.6 cycles of SIMD time whatever the occupancy; only the plain
# VOP2 adds / logic ops / moves (v_add_u32 820, v_and_b32 881, v_xor_b32 894, v_ashrrev_i32 883, v_mov_b32 980) share a
# 2-cycle slot between waves.  The roof a kernel of the first kind is priced against:
VALU_PEAK_GI = 530.0
VALU_FAST_GI = 850.0


def csrc_sha16():
    """sha256 over the kernel / shim sources of THIS tree (tools/make_pmc_traffic.py stamps profiles/pmc_traffic.json with the same)"""
    d = os.path.join(ROOT, "digital-subband-video-1_amd", "csrc")
    names = sorted(n for n in os.listdir(d) if n.endswith((".hip", ".hpp")) or n == "Makefile")
    h = hashlib.sha256()
    for n in names + [os.path.join("..", "..", "include", "dsvg_rc.h")]:
        h.update(os.path.basename(n).encode() + b"\0" + open(os.path.join(d, n), "rb").read())
    return h.hexdigest()[:16]


def traffic_stamp(T):
    """is the committed counter file older than the kernels?  (verdict round 4: it was scaled silently)"""
    now = csrc_sha16()
    return {"traffic_commit": T.get("commit", "unstamped"), "traffic_csrc_sha16": T.get("csrc_sha16", "unstamped"), "csrc_sha16": now,
            "traffic_stale": T.get("csrc_sha16") != now}


def link_rates(shard, dev, placement=None):
    """the box's host <-> device link, measured through the LIBRARY's own copy path (dsvg_link_probe: hipHostMalloc'd memory, asynchronous 1 GiB copies
    timed by HIP events, in a child process of this process's affinity) -- round 5's figure came from another allocator's pinned memory and read 29 GB/s
    on a box where the staged clip upload then ran at 37.5 (`frac_of_link` 1.29).  When the placement probe already measured the chosen placement
    before the GPU was touched, that measurement is the one reported."""
    if placement and placement.get("chosen") and placement["measured"].get(placement["chosen"]):
        return dict(placement["measured"][placement["chosen"]], source="dsvg_link_probe in a fresh child process on the chosen cores, before this process touched the GPU")
    r = shard.link_probe(dev)
    return dict(r, source="dsvg_link_probe in a child process of this process's affinity") if r else None


def dump_outputs(out_dir, outs, prefix="", budget=64 * 10 ** 6, seed=0xD5F1):
    """--dump-outputs: what the timed path handed its caller in the last timed step -- the finished .dsv bytes of every stream --
    written so that two builds can be compared output for output:
      <prefix>stream_lengths.npy  float64 [streams]   the byte length of every stream
      <prefix>stream_index.npy    float64 [k]         the streams sampled, in stream order
      <prefix>stream_bytes.npy    float32 [sum]       the bytes (0..255) of the sampled streams, concatenated in that order
    The sample is fixed: streams are taken in one seeded order while their bytes still fit, all files together within `budget`."""
    os.makedirs(out_dir, exist_ok=True)
    lengths = np.array([len(o) for o in outs], dtype=np.float64)
    room = budget - 2 * lengths.nbytes - 3 * 4096           # (the index is never longer than the lengths; .npy headers)
    take = []
    for s in np.random.default_rng(seed).permutation(len(outs)):
        if 4 * (lengths[s] + lengths[take].sum()) > room:
            break
        take.append(int(s))
    take.sort()
    data = np.concatenate([np.frombuffer(outs[s].view(), dtype=np.uint8) for s in take] or [np.empty(0, np.uint8)]).astype(np.float32)
    np.save(os.path.join(out_dir, prefix + "stream_lengths.npy"), lengths)
    np.save(os.path.join(out_dir, prefix + "stream_index.npy"), np.array(take, dtype=np.float64))
    np.save(os.path.join(out_dir, prefix + "stream_bytes.npy"), data)


def box_info():
    """what the host looked like while this ran: other tenants' load, this container's CPU quota (a box is one GPU of a shared 8-GPU host)"""
    out = {}
    try:
        out["loadavg"] = open("/proc/loadavg").read().split()[:3]
    except OSError:
        pass
    for name, path in (("cgroup_cpu_max", "/sys/fs/cgroup/cpu.max"), ("cgroup_cpuset", "/sys/fs/cgroup/cpuset.cpus.effective")):
        try:
            out[name] = open(path).read().strip()
        except OSError:
            pass
    return out


def cpu_info():
    model = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return model, os.cpu_count()


def ref_encode(pkg, A, clip, w, h, fmt, start_fnum=0, **cli):
    """one stream through the CPU checker: the REAL reference encoder (oracle/_ref, one thread) where it was built,
    else our scalar port in oracle/.  clip [frames][bytes]; returns (.dsv bytes without EOS, kind)"""
    if A.have_ref():
        L = C.CDLL(A.REF_SO)
        L.dsv_load_planar_frame.restype = C.c_void_p
        L.dsv_load_planar_frame.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.dsv_enc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        enc = pkg.make_encoder_cfg(w, h, fmt, **cli)     # same struct layout
        enc.next_fnum = start_fnum
        L.dsv_enc_start(C.byref(enc))
        out = b""
        bufs = (pkg.Buf * 4)()
        for t in range(clip.shape[0]):
            fr = L.dsv_load_planar_frame(fmt, clip[t].ctypes.data, w, h)
            nb = L.dsv_enc(C.byref(enc), fr, bufs) & 3
            for i in range(nb):
                out += C.string_at(bufs[i].data, bufs[i].len)
                L.dsv_buf_free(C.byref(bufs[i]))
        L.dsv_enc_free(C.byref(enc))
        return out, "reference"
    s, _ = A.orc_encode(clip, A.orc_cfg(w, h, fmt, **cli), start_fnum=start_fnum, eos=False)
    return s, "port"


def cpu_baseline(clips, pkg, A, reps=1):
    """time the reference encoder (1 thread) on `clips` [g][GOP][bytes], `reps` passes over them (pass r encodes
    GOP numbers r*len(clips)..); returns dict + the streams of the first pass"""
    streams = []
    nd = clips.shape[0]
    clips = np.concatenate([clips] * reps, axis=0) if reps > 1 else clips
    kind = "port"
    t0 = time.perf_counter()
    for g in range(clips.shape[0]):
        s_, kind = ref_encode(pkg, A, clips[g], W, H, FMT, start_fnum=g * GOP, qp=QP, gop=GOP, rc_mode_cli=1)
        streams.append(s_)
    dt = time.perf_counter() - t0
    mpix = clips.shape[0] * GOP * W * H / 1e6
    model, ncpu = cpu_info()
    return {"value": round(mpix / dt, 2), "unit": "Mpix/s", "cores": 1, "kind": kind, "cpu_model": model, "nproc": ncpu,
            "sample": "%d GOPs x %d frames 1920x1080 4:2:0 -gop12 -qp85 -rc_mode1 (%d distinct synthetic clips), %.1f s"
                      % (clips.shape[0], GOP, nd, dt)}, streams[:nd]


def first_picture_fnum(A, stream):
    """frame number of the first picture packet of a .dsv byte string (32 bits after the 14-byte packet header, B.2.3)"""
    for p in A.split_packets(bytes(stream)):
        if p[5] & 4:
            return int.from_bytes(p[14:18], "big")
    raise ValueError("no picture packet")


def continuing_gop(A, fresh):
    """what a closed GOP looks like when it is NOT the first of its stream, derived from a FRESH reference encode of the same
    GOP at the same frame numbers: the only field that differs is prev_link of the GOP's first picture packet, which links to
    the last packet of the GOP before (set_link_offsets, dsv_encoder.c:171-192; metadata packets carry 0).  The GOP before
    holds the same clip at other frame numbers -- a fixed 32-bit field -- so its last packet is as long as this GOP's own."""
    pk = [bytearray(p) for p in A.split_packets(fresh)]
    pics = [p for p in pk if p[5] & 4]
    pics[0][6:10] = len(pics[-1]).to_bytes(4, "big")
    return b"".join(bytes(p) for p in pk)


def joined_gops(A, fresh, ngops, gop, eos=False):
    """the serial stream of `ngops` closed GOPs that all hold the clip of `fresh` (ONE reference encode, frame numbers 0..gop-1),
    derived packet by packet: picture k of GOP g carries frame number g*gop + k (32 bits at byte 14) and prev_link = the length
    of the picture packet before it (0 for the stream's first), metadata packets carry prev_link 0 (dsv_encoder.c:171-192,804-810);
    eos: + the end-of-stream packet dsv_enc_end_of_stream appends (header only, type 0x10, next_link 0: dsv_encoder.c:766-778)"""
    out, prev = [], 0
    for g in range(ngops):
        for p in A.split_packets(fresh):
            p = bytearray(p)
            if p[5] & 4:
                p[14:18] = (int.from_bytes(p[14:18], "big") + g * gop).to_bytes(4, "big")
                p[6:10] = prev.to_bytes(4, "big")
                prev = len(p)
            out.append(bytes(p))
    if eos:
        out.append(b"DSV1" + bytes([0, 0x10]) + prev.to_bytes(4, "big") + (0).to_bytes(4, "big"))
    return b"".join(out)


def intra_block_pct(A, clip, w, h, fmt, **cli):
    """share of intra blocks in the P pictures of `clip`, from the motion fields of the oracle encoder (checker role: it
    describes the content of a shape, nothing timed goes through it)"""
    L = A.load_orc()
    cfg = A.orc_cfg(w, h, fmt, **cli)
    e = L.orc_enc_open(C.byref(cfg))
    out, n, cap = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
    intra = total = 0
    for t in range(clip.shape[0]):
        L.orc_enc_frame(e, clip[t].ctypes.data, C.byref(out), C.byref(n), C.byref(cap), None)
        cnt = C.c_int(0)
        p = L.orc_enc_last_mvs(e, C.byref(cnt))
        if t == 0 or not p or cnt.value == 0:
            continue
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cnt.value * 12,)).reshape(cnt.value, 12)
        intra += int((a[:, 4] != 0).sum())
        total += cnt.value
    C.CDLL(None).free(out)
    L.orc_enc_close(e)
    return round(100.0 * intra / max(total, 1), 1)


def shape_bench(pkg, A, dev, w, h, fmt, streams, frames, steps, seed, check_frames, style=0, count_patches=False, styles=None, **cli):
    """the same pipelined loop on another shape of BASELINE.json (dsv_main.c:463-489 flag mapping in make_encoder_cfg):
    `streams` x `frames` pictures per step, raw frames resident in HBM; CRF runs submit/collect, ABR (serial per frame)
    plain encode calls.  One stream is compared bit for bit with the CPU checker on its first `check_frames` frames."""
    fb = A.frame_bytes(w, h, fmt)
    clip = A.gen_clip(w, h, fmt, seed, frames, style=style)
    batch_in = np.empty((streams, frames, fb), dtype=np.uint8)
    if styles:
        # `styles`: one distinct clip per entry (its own seed), dealt over the streams in turn -- the batch's branch behaviour is as mixed as the list
        clips = [clip if k == 0 and st_ == style else A.gen_clip(w, h, fmt, seed + 7919 * k, frames, style=st_) for k, st_ in enumerate(styles)]
        for s_ in range(streams):
            batch_in[s_] = clips[s_ % len(clips)]
    else:
        clips = [clip]
        batch_in[:] = clip
    cfg = pkg.make_encoder_cfg(w, h, fmt, **cli)
    b = pkg.Batch(cfg, streams, frames, device=dev)
    patches = None
    try:
        d = b.upload(batch_in)
        first = b.encode(d, on_device=True)
        if count_patches:
            # what the sparse inverse kernels find in this content: the 8x8 patches of the P pictures whose detail flags are up (counted by
            # the kernels themselves in an untimed pass of their own: the counting costs atomics)
            b.tile_stats()
            b.encode(d, on_device=True)
            ts = b.tile_stats(enable=False)
            nP = streams * sum(1 for t in range(frames) if cli.get("gop", 12) > 0 and t % max(cli.get("gop", 12), 1) != 0)
            cw_, ch_ = A.chroma_dims(w, h, fmt)
            ly, lc = nP * ((w + 7) // 8) * ((h + 7) // 8), 2 * nP * ((cw_ + 7) // 8) * ((ch_ + 7) // 8)
            patches = {"flagged_patches_luma": int(ts["flagged_patches_luma"]), "patches_luma": ly,
                       "flagged_share_luma": round(ts["flagged_patches_luma"] / max(ly, 1), 4),
                       "flagged_patches_chroma": int(ts["flagged_patches_chroma"]), "patches_chroma": lc,
                       "flagged_share_chroma": round(ts["flagged_patches_chroma"] / max(lc, 1), 4)}
        crf = cli.get("rc_mode_cli", 1) == 1
        # ABR streams are pipelined like CRF ones since round 4: their rate control runs on the device (k_rc), the state goes from
        # call to call there, so the analysis of batch i + 1 overlaps the coding of batch i (DSV1_ABR_SERIAL=1: plain encode calls)
        piped = crf or os.environ.get("DSV1_ABR_SERIAL", "0") in ("", "0")
        if piped:
            b.submit(d, on_device=True, held=True)                  # fill the pipeline (as the headline loop does)
        b.sync()
        t0 = time.perf_counter()
        if piped:
            for _ in range(steps):
                b.submit(d, on_device=True, held=True)
                outs = b.collect(copy=False)
            b.sync()
            dt = time.perf_counter() - t0
            b.collect(copy=False)
            n = steps
        else:
            for _ in range(steps):
                outs = b.encode(d, on_device=True)
            b.sync()
            dt = time.perf_counter() - t0
            n = steps
    finally:
        b.close()
    res = {"ms_per_step": round(1e3 * dt / n, 3), "Mpix_s": round(n * streams * frames * w * h / dt / 1e6, 1),
           "frames_per_s": round(n * streams * frames / dt, 1), "pictures_per_step": streams * frames,
           "dsv_bytes_per_step": int(sum(len(o) for o in outs))}
    if patches:
        res.update(patches)
    if check_frames:
        # a fresh single-stream GPU encode of the first check_frames frames against the CPU checker
        got = pkg.encode_clip(clip[:check_frames], w, h, fmt, device=dev, eos=False, **cli)
        want, kind = ref_encode(pkg, A, clip[:check_frames], w, h, fmt, **cli)
        res["bit_exact_vs_cpu"] = bool(got == want)
        res["checked"] = "%d frames, 1 stream, vs %s" % (check_frames, kind)
        # ... and the batch's own first stream starts with the same packets (CRF: streams are independent of the batch)
        if crf and check_frames >= frames:
            res["bit_exact_vs_cpu"] = res["bit_exact_vs_cpu"] and bytes(first[0]) == want
            if styles:
                # ... and three more of the distinct clips, each against the reference's encode of that clip
                nc = min(len(clips), streams)
                ks = sorted(set((nc // 3, 2 * nc // 3, nc - 1)) - {0})
                for k in ks:
                    wk, _ = ref_encode(pkg, A, clips[k], w, h, fmt, **cli)
                    res["bit_exact_vs_cpu"] = res["bit_exact_vs_cpu"] and bytes(first[k]) == wk
                res["checked"] += "; the batch's streams 0, %s vs the reference's encodes of their clips" % ", ".join(str(k) for k in ks)
    return res


def cfg4_sharded(pkg, A, shard, torch, dist, dev, rank, world, shared, steps, ngops):
    """BASELINE config 4 as it is written: `ngops` (64) closed 3840x2160 4:2:0 GOPs of 12 frames sharded over the ranks by
    shard.gop_range (8 per GPU on a full node), no data-path collective.  Every rank codes its GOPs with their frame numbers;
    a step = all `ngops` GOPs once, timed like the headline (barrier + sync on both sides, MAX over ranks).  The streams of the
    first pass are gathered on rank 0 (host bytes), joined by dsv1_concat_gops and compared with the serial stream derived from
    ONE reference encode of the GOP clip (joined_gops).  Collective: every rank calls it."""
    w, h, fmt, gop = 3840, 2160, 0x5, 12
    lo, hi = shard.gop_range(ngops, world, rank)
    n = hi - lo
    clip = A.gen_clip(w, h, fmt, 0x21600004, gop, style=0)
    cli = dict(qp=85, gop=gop, rc_mode_cli=1, scd=0)
    tmax, first = 0.0, []
    b, err = None, None
    # The leg is a collective (barrier, all_reduce, gather): a rank whose set-up fails (out of memory in Batch(), a failed upload)
    # must not leave the others waiting in one.  Every rank reports its set-up, all agree to run or to skip (advisor round 4).
    try:
        if n > 0:
            batch_in = np.empty((n, gop, A.frame_bytes(w, h, fmt)), dtype=np.uint8)
            batch_in[:] = clip
            b = pkg.Batch(pkg.make_encoder_cfg(w, h, fmt, **cli), n, gop, device=dev)
            d = b.upload(batch_in)
            for s_ in range(n):
                b.set_fnum(s_, (lo + s_) * gop)
            first = [(lo + s_, bytes(o)) for s_, o in enumerate(b.encode(d, on_device=True))]
            b.submit(d, on_device=True, held=True)
            b.sync()
    except Exception as e:          # noqa: BLE001 -- reported, and agreed on below
        err = "rank %d: %s: %s" % (rank, type(e).__name__, e)
    if world > 1:
        ok = torch.tensor([0 if err else 1], dtype=torch.int32, device="cpu" if shared else "cuda")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        all_ok = bool(ok.item())
    else:
        all_ok = err is None
    if not all_ok:
        if b is not None:
            try:
                b.close()
            except Exception:       # noqa: BLE001
                pass
        if err:
            print("[bench] cfg4_sharded skipped: " + err, file=sys.stderr)
        return {"skipped": err or "another rank failed its set-up"} if rank == 0 else None
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:                            # (a rank that fails here still meets the others in the barrier and the reductions below)
        if n > 0:
            for _ in range(steps):
                b.submit(d, on_device=True, held=True)
                b.collect(copy=False)
            b.sync()
    except Exception as e:          # noqa: BLE001
        err = "rank %d: %s: %s" % (rank, type(e).__name__, e)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    tmax = time.perf_counter() - t0
    try:
        if n > 0 and not err:
            b.collect(copy=False)
    except Exception as e:          # noqa: BLE001
        err = "rank %d: %s: %s" % (rank, type(e).__name__, e)
    finally:
        if n > 0:
            try:
                b.close()
            except Exception:       # noqa: BLE001
                pass
    if world > 1:
        t = torch.tensor([tmax, 1.0 if err else 0.0], dtype=torch.float64, device="cpu" if shared else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tmax, failed = float(t[0].item()), bool(t[1].item())
    else:
        failed = err is not None
    if failed:
        if err:
            print("[bench] cfg4_sharded failed: " + err, file=sys.stderr)
        return {"error": err or "another rank failed in the timed region"} if rank == 0 else None
    parts = shard.gather_streams(first, dist if world > 1 else None)
    if rank != 0:
        return None
    joined = pkg.concat_gops(parts)
    fresh, kind = ref_encode(pkg, A, clip, w, h, fmt, **cli)
    want = joined_gops(A, fresh, ngops, gop, eos=True)          # (dsv1_concat_gops ends the joined stream)
    return {"config": "3840x2160 4:2:0 -gop12 -qp85 -rc_mode1 -scd0, %d closed GOPs x 12 frames per step sharded over %d rank(s) by shard.gop_range "
                      "(%d per GPU), no data-path collective; raw frames resident in HBM" % (ngops, world, -(-ngops // world)),
            "Mpix_s": round(steps * ngops * gop * w * h / tmax / 1e6, 1), "ms_per_step": round(1e3 * tmax / steps, 3), "steps": steps,
            "gops": ngops, "gops_per_gpu": -(-ngops // world), "n_gpus": world,
            "joined_stream_bytes": len(joined), "sha256": hashlib.sha256(joined).hexdigest(), "sha256_expected": hashlib.sha256(want).hexdigest(),
            "bit_exact_vs_cpu": bool(joined == want),
            "checked": "the %d gathered GOPs joined by dsv1_concat_gops vs the serial stream derived from one %s encode of the GOP clip "
                       "(frame numbers and prev_link rewritten per packet, dsv_encoder.c:171-192)" % (ngops, kind)}


def decode_bench(pkg, A, dev, streams, reps):
    """batched decoder (dsv1_decbatch_*): `streams` copies of a 1080p GOP=12 stream side by side, one packet of each per
    call, decoded frames left in HBM; every frame of stream 0 compared with the oracle decoder's"""
    clip = A.gen_clip(W, H, FMT, 0x10800003, GOP, style=0)
    stream = pkg.encode_clip(clip, W, H, FMT, device=dev, qp=QP, gop=GOP, rc_mode_cli=1)
    pk = A.split_packets(stream)
    want = A.orc_decode(stream, W, H, FMT)
    d = pkg.DecBatch(W, H, FMT, streams, device=dev)
    try:
        ok = True
        k = 0
        for p in pk:                                     # checked pass (host output of stream 0)
            _, status, fnum = d.decode([p] * streams, on_device=True)
            if status[0] == 0 and (p[5] & 4):
                got = d.download()
                ok = ok and k < len(want) and bool((got[0] == want[k]).all()) and bool((got[streams - 1] == want[k]).all())
                k += 1
        ok = ok and k == len(want)
        # timed passes: the packet tables are built once (the C entry point is called directly, as a C caller would)
        L = pkg.lib()
        keep = [np.frombuffer(bytes(p) + b"\0" * 16, dtype=np.uint8).copy() for p in pk]
        calls = []
        for kk, p in enumerate(pk):
            bufs = (pkg.Buf * streams)()
            for s_ in range(streams):
                bufs[s_].data = keep[kk].ctypes.data_as(C.POINTER(C.c_uint8))
                bufs[s_].len = len(p)
            calls.append(bufs)
        status = (C.c_int * streams)()
        fnum = (C.c_uint32 * streams)()
        npic = sum(1 for p in pk if p[5] & 4)
        d.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            for bufs in calls:
                rc = L.dsv1_decbatch_decode(d.h, bufs, d._dev, d.frame_bytes, 1, status, fnum)
                if rc != 0:
                    raise RuntimeError("dsv1_decbatch_decode rc=%d: %s" % (rc, L.dsvg_last_error().decode()))
        d.sync()
        dt = time.perf_counter() - t0
        n = reps * npic * streams
    finally:
        d.close()
    return {"Mpix_s": round(n * W * H / dt / 1e6, 1), "frames_per_s": round(n / dt, 1), "streams": streams,
            "ms_per_call": round(1e3 * dt / (reps * len(pk)), 3), "bit_exact_vs_cpu": ok,
            "checked": "%d frames of streams 0 and %d vs the oracle decoder" % (len(want), streams - 1),
            "output": "decoded frames left in HBM (packed planar)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150, help="timed steps (default: a timed region of ~5 s, so that coarse GPU-busy sampling around the run can see it)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gops", type=int, default=320, help="closed GOPs per GPU per step (320 GOPs keep ~100 GB of HBM and 12 GB of host memory; tools/ab/gops_sweep.sh "
                                                          "measures other sizes on the same box -- DESIGN.md section 7 has the round's table)")
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic GOP clips generated per rank (round 6: 16, was 4 -- the timed batch's branch behaviour is 16-valued; "
                                                                 "every one of them is checked against the reference's encode; `shapes.headline_mixed16` mixes clip STYLES as well)")
    ap.add_argument("--full", action="store_true", help="besides the headline, everything else the benchmark measures or checks: the NUMA placement measured over the link, "
                                                        "the per-kernel roofline, the CPU baseline and the bit-exact checks against the reference, and (unless --no-extras) "
                                                        "the every-picture-reconstructed loop, the host-fed figure, the other shapes and config 4's sharded leg")
    ap.add_argument("--cpu-gops", type=int, default=32, help="with --full: GOP encodes in the CPU baseline sample, ~0.3 s each (0 = skip the baseline and the bit-exact checks)")
    ap.add_argument("--prof-kernel", default="auto", help="with --full: kernel whose launches are timed with HIP events (auto = the largest; none = no brackets, no roofline: counter passes)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the PCIe-inclusive figure and the other shapes (configs 2, 4, 5, batched decode) reported after the headline")
    ap.add_argument("--cfg4-gops", type=int, default=64, help="with --full: closed 4K GOPs of the config-4 leg that runs sharded over the ranks when --gpus > 1 (or with --cfg4-sharded); 0 = skip")
    ap.add_argument("--cfg4-sharded", action="store_true", help="with --full: run the sharded config-4 leg on one GPU too (all its GOPs on this GPU)")
    ap.add_argument("--input", choices=["hbm", "host", "pinned"], default="hbm",
                    help="where the raw frames are when a step starts: hbm (the metric), or host memory (pageable / pinned) "
                         "uploaded over PCIe inside the timed region (diagnostic, DESIGN.md section 7)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the .dsv bytes the last timed step returned to DIR/*.npy "
                                                          "(every stream's length and a fixed sample of the streams, at most 64 MB; see dump_outputs)")
    args = ap.parse_args()

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if not args.full and (args.cfg4_sharded or args.prof_kernel not in ("auto", "none")):
        ap.error("--cfg4-sharded and --prof-kernel <name> ask for legs of a --full run")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started plainly with --gpus N: be the launcher (verdict round 5: the flag was parsed and never used).  Nothing has touched the
        # GPU yet, and the ranks are CHILDREN of this process (one per GPU, torch.distributed.run over 127.0.0.1), never an exec.
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks: the line would claim the wrong n_gpus" % (args.gpus, world))
    # one process per GPU: before anything touches the GPU, take this rank's share of the host cores (the session
    # layer's worker threads, the runtime's helper threads and the first touch of the pinned buffers stay on it)
    shard = importlib.import_module("digital-subband-video-1_amd.shard")
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    my_cores = shard.pin_rank_to_cores(local_rank, local_world)
    numa_node = None
    placement = None
    if local_world <= 1 and os.environ.get("DSV1_BENCH_NO_NUMA_PIN", "0") in ("", "0"):
        # one process, one GPU: onto the cores of the GPU's NUMA node before anything touches the GPU (round 5; the host-fed figures depend on it)
        forced = os.environ.get("DSV1_BENCH_NUMA_NODE")            # diagnostic: pin to THIS node whatever sysfs says (tools/ab/r06_repro.sh)
        if forced not in (None, ""):
            my_cores, numa_node = shard.pin_single_rank(local_rank, node=int(forced))
        elif not args.full or os.environ.get("DSV1_BENCH_SYSFS_PIN", "0") not in ("", "0"):
            my_cores, numa_node = shard.pin_single_rank(local_rank)       # round 5: trust sysfs (a plain run: the node sysfs names, no link measured)
        else:
            # round 6: ask the LINK -- the host <-> device rates from fresh child processes on the sysfs node's cores, on the other node's, and
            # unpinned, before this process touches the GPU; the process moves to the best (the sysfs node unless another is > 5 % better)
            my_cores, numa_node, placement = shard.pin_single_rank_measured(local_rank)
    import torch
    import torch.distributed as dist
    # debugging aid for boxes with fewer GPUs than ranks (never set by the driver): all ranks share device 0 and the
    # two collectives of this script (barrier, MAX of the elapsed time) go over gloo
    shared = os.environ.get("DSV1_BENCH_DEBUG_SHARED_GPU") == "1"
    dev = 0 if shared else local_rank
    torch.cuda.set_device(dev)
    if world > 1:
        if shared:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import _cabi as A
    pkg = importlib.import_module("digital-subband-video-1_amd")
    L = pkg.lib()                                   # raises if the HIP extension is missing
    if L.dsvg_device_count() < 1:
        raise RuntimeError("no HIP device: the product path has no CPU fallback")

    # synthetic input (integer generator, throughput style: pan + texture)
    nd = max(1, min(args.distinct, args.gops))
    fb = A.frame_bytes(W, H, FMT)
    distinct = np.empty((nd, GOP, fb), dtype=np.uint8)
    for g in range(nd):
        distinct[g] = A.gen_clip(W, H, FMT, 0x10800003 + 977 * rank + g, GOP, style=0)
    batch_in = np.empty((args.gops, GOP, fb), dtype=np.uint8)
    for s in range(args.gops):
        batch_in[s] = distinct[s % nd]

    cfg = pkg.make_encoder_cfg(W, H, FMT, qp=QP, gop=GOP, rc_mode_cli=1)
    b = pkg.Batch(cfg, args.gops, GOP, device=dev)
    if args.input == "hbm":
        src, ondev = b.upload(batch_in), True       # raw clip resident in HBM before any timing
    else:
        if args.input == "pinned":
            host = b.pinned(batch_in.shape)
            host[...] = batch_in
            batch_in = host
        src, ondev = batch_in, False

    def sync_all():
        if world > 1:
            dist.barrier()
        b.sync()
        torch.cuda.synchronize()

    # Steps are software-pipelined (dsv1_batch_submit / dsv1_batch_collect): one step = collect batch i
    # (gathered D2H + host packet assembly) + submit batch i+1 (analysis on the second HIP stream overlaps
    # the residual coding of batch i).  Exactly one full batch of work per step, one batch in flight at the
    # region boundaries (its device part is synchronised on both sides).
    outs = None
    for _ in range(max(args.warmup, 1)):
        outs = b.encode(src, on_device=ondev)
    # pick the kernel to time: one untimed step with every kernel bracketed, on ONE coding stream so that each kernel
    # has the chip to itself while it is measured (the timed region below runs the default two coding streams: there a
    # launch covers half of the pictures and shares the chip with the other half's kernels); take the largest total
    names = b.kernel_names()
    table = {}
    tiles = None
    prof_kernel = args.prof_kernel
    nstreams = b.code_streams(0)
    if rank == 0 and prof_kernel != "none" and not args.full:
        # a plain run codes the two untimed steps below unmeasured, so that its timed steps code the same frame numbers -- and
        # therefore the same bytes -- as a --full run's; no kernel is selected, no launch of the timed region is bracketed
        for _ in range(2):
            b.encode(src, on_device=ondev)
        prof_kernel = "none"
    if rank == 0 and prof_kernel != "none":     # "none": no event brackets at all (the counter passes of tools/collect_profiles.sh)
        b.code_streams(1)
        b.prof_enable(names)
        b.encode(src, on_device=ondev)
        b.sync()
        table = {k: b.prof_get(k) for k in names}
        # ... and one more untimed step that COUNTS what the sparse inverse kernels moved (tiles, flagged patches): the counting
        # costs atomics, so it has a step of its own and no kernel is timed while it is on
        b.prof_enable([])
        b.tile_stats()
        b.encode(src, on_device=ondev)
        b.sync()
        tiles = b.tile_stats(enable=False)
        # the sparse inverse transform moves data only for tiles that carry a residual: price it at what it really moved
        # (general tile: 128x64 samples x 2.5 B = prediction 1 + reconstruction 1 + level-2/3 symbols 0.47 + flags; the level-1
        # symbols are only fetched for flagged patches; every tile: its 20x12 LL3 values and patch flags, 5 B each)
        # The tiles away from the right / bottom edge run in k_inv_p_tile<true>, the strips in k_inv_haar_tile<true, 0, true>
        # (launch_inv_sbt): the counted tiles are shared out by the grid's geometry.
        w3, h3 = (W + 7) >> 3, (H + 7) >> 3
        ntx, nty = (w3 + 15) // 16, (h3 + 7) // 8
        fx = (w3 - 18) // 16 + 1 if w3 >= 18 else 0
        if fx == ntx - 1 and w3 == 16 * ntx and W % 8 == 0:
            fx += 1                                 # the last tile column ends with the band: the fast kernel's edge body takes it
        fy = (h3 - 10) // 8 + 1 if h3 >= 10 else 0
        if fy == nty - 1 and H % 8 == 0:
            fy += 1                                 # ... and the last tile row
        ffast = (fx * fy) / float(ntx * nty)
        # Round 4: + the level-1 symbols of the patches whose flag is up (96 bytes per 8x8 patch, counted by the kernel itself in this
        # step: `flagged_patches_luma`) -- input the kernel cannot avoid reading, which the figure left out until now while the
        # counters showed it (round 3: 24.9 GB by counters against 19.5 GB priced).
        for kname, share in (("void k_inv_p_tile<true>", ffast), ("void k_inv_haar_tile<true, 0, true>", 1.0 - ffast)):
            tg, tz = tiles["general_luma"] * share, tiles["zero_luma"] * share
            if kname in table and table[kname][1]:
                m_, n_, _ = table[kname]
                sym1 = tiles["flagged_patches_luma"] * 96.0 if kname == "void k_inv_p_tile<true>" else 0.0
                table[kname] = (m_, n_, tg * 128.0 * 64.0 * 2.5 + (tg + tz) * 240.0 * 5.0 + sym1)
        # the chroma patch kernel likewise at what it moved: LL3 value + flag of every patch (5 B), prediction in / reconstruction out
        # (128 B) of the patches it rewrote, and the symbols of the three levels (16 + 4 + 1 cells x 3 bands x 2 B = 126 B) of the flagged ones
        kname = "k_inv_patch_c"
        if kname in table and table[kname][1]:
            m_, n_, by_ = table[kname]
            npatch = by_ / 128.0
            fl, mv = tiles["flagged_patches_chroma"], tiles["moved_unflagged_patches_chroma"]
            # round 6: + the reconstruction borders the kernel writes for all three planes (fused border, by the extents the motion vectors ask for:
            # `fused_border_bytes`, tallied on the host from the jobs' extents in the same counting step) -- output it cannot avoid writing
            table[kname] = (m_, n_, npatch * 5.0 + (fl + mv) * 128.0 + fl * 126.0 + float(tiles.get("fused_border_bytes", 0)))
        if prof_kernel == "auto":
            # the largest of the kernels whose bytes are priced: on small batches the top kernels are within a percent of each other, and
            # one without algorithmic bytes (k_fwd_mc_pix) would put the roofline at 0
            priced = [k for k in table if table[k][2] > 0] or list(table)
            prof_kernel = max(priced, key=lambda k: table[k][0])
        b.code_streams(nstreams)
        b.prof_enable([prof_kernel])
    b.submit(src, on_device=ondev, held=True)                  # fill the pipeline
    sync_all()
    dropped0 = b.dropped_recons()[0]
    if rank == 0:
        b.breakdown_start()                         # ten HIP events and a dozen clock reads per batch (DSV1_BENCH_NO_BREAKDOWN has no A/B difference: DESIGN.md section 7)
    b.mark(0)
    t0 = time.perf_counter()
    if not ondev:
        b.stage(src)                                # host input: K uploads inside the timed region, queued back to back
    for i in range(args.steps):
        if not ondev and i + 1 < args.steps:
            b.stage(src)                            # the next step's upload follows this one's on the copy stream
        b.submit(src, on_device=ondev, held=True)
        outs = b.collect(copy=False)                # the finished packets stay in the buffers they were assembled in
    b.mark(1)                                       # (behind the last step's coding work on the first coding stream, which joins the others)
    sync_all()
    dt = time.perf_counter() - t0
    dropped_per_step = (b.dropped_recons()[0] - dropped0) / float(max(args.steps, 1))
    gpu_ms = b.mark_ms()                            # the same region by HIP events on the device
    breakdown = b.breakdown_stop(args.steps) if rank == 0 else None
    # the bytes the LAST TIMED step produced (all streams, in stream order), hashed before anything reuses their buffers;
    # compared further down with bytes derived from the reference encoder's output for the same clips and frame numbers
    timed_sha = timed_fnum = None
    if rank == 0 and args.full:
        hh = hashlib.sha256()
        for o in outs:
            hh.update(o.view())
        timed_sha = hh.hexdigest()
        timed_fnum = first_picture_fnum(A, outs[0].view())
    if args.dump_outputs:
        # every rank writes its own streams (rank-prefixed names when there are several), the 64 MB shared out among them
        dump_outputs(args.dump_outputs, outs, prefix="rank%d_" % rank if world > 1 else "", budget=64 * 10 ** 6 // world)
    b.collect(copy=False)                           # drain
    # the same loop with EVERY reference picture reconstructed (verdict round 5: the headline drops the inverse transform of each closed GOP's
    # last picture -- 320 of 3 840 --, which nobody predicts from; same packets): a few steps, never `value`
    recon_all = None
    if rank == 0 and world == 1 and args.full and not args.no_extras and args.input == "hbm":
        b.sync()
        b.recon_all(True)
        b.submit(src, on_device=True, held=True)
        b.sync()
        ra_steps = max(2, min(args.steps, 20))      # (the region ends with a sync that drains the last batch: over 8 steps that tail read as +2.5 ms per step)
        t1 = time.perf_counter()
        for _ in range(ra_steps):
            b.submit(src, on_device=True, held=True)
            ra_outs = b.collect(copy=False)
        b.sync()
        dtr = time.perf_counter() - t1
        hr = hashlib.sha256()
        for o in ra_outs:
            hr.update(o.view())
        ra_fnum = first_picture_fnum(A, ra_outs[0].view())
        b.collect(copy=False)
        b.recon_all(False)
        recon_all = {"value": round(args.gops * GOP * W * H * ra_steps / dtr / 1e6, 1), "unit": "Mpix/s", "ms_per_step": round(1e3 * dtr / ra_steps, 3), "steps": ra_steps,
                     "sha256_last_step": hr.hexdigest(), "first_frame_number": ra_fnum,
                     "note": "dsv1_batch_recon_all(1): every reference picture reconstructed, as the reference encoder does (dsv_encoder.c:665-708)"}
        del ra_outs
    kinfo = None
    if rank == 0 and prof_kernel != "none":
        whole_step = False
        ms, nl, by = b.prof_get(prof_kernel)
        b.prof_enable([])
        if prof_kernel in table and table[prof_kernel][1] and nl:
            # the algorithmic bytes of a launch as the selection step priced them (for the sparse inverse kernels: what the counted
            # tiles and flagged patches really moved), shared out over the launches the timed region needs for the same pictures
            # (a coding-stream kernel's launch covers 1 / coding_streams of a frame step there; an analysis kernel's the whole step)
            xm_, xn_, xb_ = table[prof_kernel]
            by = xb_ * (args.steps + 1)                   # (the brackets also cover the batch that fills the pipeline)
            whole_step = abs(nl / float(args.steps + 1) - xn_) < 0.5      # as many launches per step as with one coding stream: an analysis-stream kernel
        ach = by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        kinfo = {"kernel": prof_kernel, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None, "launches": nl,
                 "avg_launch_us": round(1000.0 * ms / max(nl, 1), 2),
                 "alg_bytes_per_launch": round(by / max(nl, 1)),
                 "coding_streams": nstreams,
                 "regime": "timed region: %d coding streams + the analysis and fetch streams share the chip (%s)" % (
                     nstreams, "a kernel of the analysis stream: a launch covers all pictures of a step" if whole_step else "a launch covers 1/%d of a frame step's pictures" % nstreams),
                 "all_kernels_ms_one_step_regime": "exclusive: one coding stream, the untimed selection step, each kernel alone on the chip",
                 "all_kernels_ms_one_step": {k: round(v[0], 3) for k, v in table.items() if v[1]},
                 "sparse_inverse_tiles_one_step": tiles}
        # the other large kernels, each alone on the chip (same untimed step): algorithmic bytes / HIP-event time
        oth = []
        for k, (m_, n_, b_) in sorted(table.items(), key=lambda kv: -kv[1][0]):
            if k != prof_kernel and n_ and m_ > 0 and b_ > 0 and len(oth) < 6:
                a_ = b_ / (m_ * 1e-3) / 1e9
                oth.append({"kernel": k, "achieved": round(a_, 1), "frac": round(a_ / HBM_PEAK_GBS, 4), "avg_launch_us": round(1000.0 * m_ / n_, 2),
                            "ms_one_step": round(m_, 3), "regime": "exclusive (one coding stream, untimed selection step)"})
        kinfo["others_exclusive"] = oth
        if prof_kernel in table and table[prof_kernel][0] > 0:
            xm, xn, xb = table[prof_kernel]         # the same kernel alone on the chip (one coding stream, untimed step)
            xa = xb / (xm * 1e-3) / 1e9
            kinfo["exclusive"] = {"achieved": round(xa, 1), "frac": round(xa / HBM_PEAK_GBS, 4), "launches": xn,
                                  "avg_launch_us": round(1000.0 * xm / max(xn, 1), 2), "alg_bytes_per_launch": round(xb / max(xn, 1)),
                                  "regime": "exclusive (one coding stream, untimed selection step)",
                                  "note": "one coding stream: the kernel has the chip to itself; `achieved` above is measured in the timed region, where two coding streams overlap"}

        # HBM traffic of that kernel: PMC counters cannot be read from inside this process, so the figure comes
        # from the committed rocprofv3 --pmc passes over this same command (tools/collect_profiles.sh ->
        # tools/make_pmc_traffic.py -> profiles/pmc_traffic.json), scaled to this run's GOPs per step.
        tp = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tp):
            T = json.load(open(tp))
            e = T.get("kernels", {}).get(prof_kernel)
            if e and "hbm_bytes_per_launch" in e:
                kinfo["traffic"] = round(e["hbm_bytes_per_launch"] * args.gops / T["gops"])
                if "hbm_bytes_per_launch_raw" in e:      # FETCH_SIZE + WRITE_SIZE as reported, no read-side doubling
                    kinfo["traffic_raw"] = round(e["hbm_bytes_per_launch_raw"] * args.gops / T["gops"])
                kinfo["traffic_source"] = T.get("source", "profiles/pmc_traffic.json")
                kinfo.update(traffic_stamp(T))
            if e and e.get("valu_insts_per_launch") and ms > 0:
                # integer/byte kernels can be bound by VALU issue rather than HBM: wave64 instructions of the kinds used here
                # issue at VALU_PEAK_GI chip-wide (measured, see the constant)
                vi = e["valu_insts_per_launch"] * args.gops / T["gops"]
                kinfo["valu_issue"] = {"wave_instr_per_launch": round(vi), "busy_frac": round(vi / (VALU_PEAK_GI * 1e9 * (ms * 1e-3 / max(nl, 1))), 3),
                                       "source": "SQ_INSTS_VALU, profiles/pmc_traffic.json; peak from profiles/r03_valu_rates.txt"}
                if e.get("valu_busy_by_counters") is not None:
                    # the same question answered by the counters alone (cycles with a VALU instruction in flight / SIMD cycles, the
                    # kernel alone on the chip under the profiler)
                    kinfo["valu_issue"]["busy_frac_by_counters"] = e["valu_busy_by_counters"]
                    kinfo["valu_issue"]["salu_busy_frac_by_counters"] = e.get("salu_busy_by_counters")
                if prof_kernel in table and table[prof_kernel][0] > 0:
                    # the same instructions against the time the kernel needs alone on the chip (one step of the untimed
                    # selection pass): what bounds the kernel itself, without the other coding stream's share
                    per_step = vi * nl / (args.steps + 1)          # the brackets also cover the batch that fills the pipeline
                    kinfo["valu_issue"]["busy_frac_exclusive"] = round(per_step / (VALU_PEAK_GI * 1e9 * table[prof_kernel][0] * 1e-3), 3)
                # which roof is the kernel under?  Integer kernels that read each byte once and do a lot with it (the
                # motion search: 15 candidate SADs, the half-pel lattice and the block statistics per block) sit under the
                # VALU issue roof, not the HBM one: the second entry prices the kernel against that roof, and `bound`
                # names the closer one (achieved / peak / frac stay the HBM view the contract asks for)
                vfrac = kinfo["valu_issue"]["busy_frac"]
                kinfo["valu_roof"] = {"bound": "valu", "achieved": round(vfrac * VALU_PEAK_GI, 1), "peak": VALU_PEAK_GI, "unit": "G wave-instr/s", "frac": vfrac,
                                      "frac_exclusive": kinfo["valu_issue"].get("busy_frac_exclusive"),
                                      "peak_source": "measured: tools/ubench/valu_rates.hip -> profiles/r03_valu_rates.txt (integer / byte / packed-16 forms at 8 waves per SIMD; "
                                                     "plain VOP2 add / logic / move forms reach %.0f)" % VALU_FAST_GI}
                kinfo["binding_roof"] = "valu" if max(vfrac, kinfo["valu_roof"]["frac_exclusive"] or 0.0) > kinfo["frac"] else "hbm"
                kinfo["bound"] = kinfo["binding_roof"]
                kinfo["quoted_against"] = "hbm (achieved / peak / frac); valu_roof holds the other roof"

    # ---- after the headline, outside its timed region: the same loop fed from pinned HOST memory ("frames
    # pre-loaded in host RAM"; the upload of each batch over PCIe rides inside the step), never `value`
    extras = rank == 0 and world == 1 and args.full and not args.no_extras and args.input == "hbm" and os.environ.get("DSV1_BENCH_SKIP_SHAPES") != "1"
    host_pinned = None
    link = None
    if extras:
        link = link_rates(shard, dev, placement)
        ps = 6
        host = b.pinned(batch_in.shape)
        host[...] = batch_in
        # two untimed steps first: both of the context's ingest buffers (11.9 GB each) are allocated by then -- an allocation inside the timed
        # steps cost the leg 50-500 ms of its 1.3 s (0.70-0.95 of the link from run to run for a loop whose steady period is the link's)
        b.stage(host)
        b.submit(host)
        for i in range(2):
            b.stage(host)
            b.submit(host)
            b.collect(copy=False)
        b.sync()
        t1 = time.perf_counter()
        b.stage(host)
        for i in range(ps):
            if i + 1 < ps:
                b.stage(host)
            b.submit(host)
            b.collect(copy=False)
        b.sync()
        dth = time.perf_counter() - t1
        b.collect(copy=False)
        host_pinned = {"value": round(args.gops * GOP * W * H * ps / dth / 1e6, 1), "unit": "Mpix/s", "ms_per_step": round(1e3 * dth / ps, 3),
                       "steps": ps, "note": "same workload, raw frames in pinned host memory, one %.2f GB upload per step inside the step (double-buffered ingest)"
                                            % (batch_in.nbytes / 1e9),
                       # the step moves its raw frames host -> device: that rate against the link's own (measured in this run, same process, same NUMA placement)
                       "upload_GBs": round(batch_in.nbytes * ps / dth / 1e9, 2), "link_GBs": link["h2d_GBs"] if link else None,
                       "frac_of_link": round(batch_in.nbytes * ps / dth / 1e9 / link["h2d_GBs"], 3) if link else None}
        del host

    tmax = dt
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if shared else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tmax = float(t.item())
    pix_per_step = args.gops * GOP * W * H
    value = world * pix_per_step * args.steps / tmax / 1e6

    # parity spot check + CPU baseline on rank 0 only
    cpu = None
    bit_exact = None
    timed_check = None
    if rank == 0:
        ncpu = min(args.cpu_gops, nd) if args.full else 0
        if ncpu > 0:
            # fresh GPU streams for the same GOP clips with the same frame numbers as the CPU run -- 16 of them (every
            # clip several times) so that the check goes through the same two-coding-stream path as the timed region
            nchk = max(16, ncpu)
            chk = pkg.Batch(cfg, nchk, GOP, device=dev)
            for s in range(nchk):
                chk.set_fnum(s, (s % ncpu) * GOP)
            gpu_streams = chk.encode(np.stack([distinct[s % ncpu] for s in range(nchk)]))
            chk.close()
            # the timed CPU sample is reported at N=1 only; at N>1 one pass still serves as the parity spot check
            cpu, cpu_streams = cpu_baseline(distinct[:ncpu], pkg, A, reps=max(1, args.cpu_gops // ncpu) if world == 1 else 1)
            bit_exact = all(gpu_streams[s] == cpu_streams[s % ncpu] for s in range(nchk))
            # ... and the output of the last TIMED step itself: every stream of that batch is GOP number timed_fnum / 12 of its
            # stream, so the expected bytes are the reference's encode of the same clip at those frame numbers, as a GOP
            # that continues a stream (continuing_gop)
            want = [continuing_gop(A, ref_encode(pkg, A, distinct[g], W, H, FMT, start_fnum=timed_fnum, qp=QP, gop=GOP, rc_mode_cli=1)[0]) for g in range(nd)]
            hw = hashlib.sha256()
            for s in range(args.gops):
                hw.update(want[s % nd])
            timed_check = {"sha256": timed_sha, "sha256_expected": hw.hexdigest(), "equal": timed_sha == hw.hexdigest(), "streams": args.gops,
                           "first_frame_number": timed_fnum,
                           "expected_from": "the reference encoder (%s) on the %d distinct clips at the timed step's frame numbers; prev_link of each GOP's first "
                                            "picture packet set to the length of the GOP's last packet (the GOP before holds the same clip)" % (cpu["kind"], nd)}
            bit_exact = bit_exact and timed_check["equal"]
            if recon_all:
                want_r = [continuing_gop(A, ref_encode(pkg, A, distinct[g], W, H, FMT, start_fnum=recon_all["first_frame_number"], qp=QP, gop=GOP, rc_mode_cli=1)[0]) for g in range(nd)]
                hw = hashlib.sha256()
                for s in range(args.gops):
                    hw.update(want_r[s % nd])
                recon_all["bit_exact_vs_cpu"] = recon_all["sha256_last_step"] == hw.hexdigest()
                bit_exact = bit_exact and recon_all["bit_exact_vs_cpu"]
            if world > 1:
                cpu = None
        out_bytes = sum(len(o) for o in outs)
        res = {
            "metric": "encoded Mpixels/sec, 1080p 4:2:0 GOP=12, bit-exact .dsv",
            "value": round(value, 2),
            "unit": "Mpix/s",
            "n_gpus": world,
            "steps": args.steps,
            "full": args.full,
            "timed_region": {"host_clock_s": round(dt, 4), "gpu_events_s": round(gpu_ms / 1e3, 4),
                             "note": "the K timed steps by the host clock (barrier + sync on both sides: what `value` uses) and by HIP events recorded on the first "
                                     "coding stream at the region's start and behind its last coding work"},
            "step_breakdown": breakdown,
            "box": dict(box_info(), placement=placement),
            "value_recon_all": recon_all,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * tmax / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8/int16+int32 (bit-exact; packed int16 inside a proven range, int32 escape)",
            "data": "synthetic",
            "config": {"workload": "1920x1080 4:2:0 GOP=12 CRF qp85, %d closed GOPs (x12 frames) per GPU per step, %s, output = finished .dsv packets"
                       % (args.gops, {"hbm": "raw frames resident in HBM", "host": "raw frames uploaded from pageable host memory each step (PCIe inclusive, diagnostic)",
                                      "pinned": "raw frames uploaded from pinned host memory each step (PCIe inclusive, diagnostic)"}[args.input]),
                       "gops_per_gpu": args.gops, "frames_per_step": args.gops * GOP * world,
                       "dsv_bytes_per_step_rank0": out_bytes, "parallelism": "gop-shard x%d, no collectives" % world,
                       "host_cores_rank0": len(my_cores), "host_threads_rank0": L.dsv1_host_threads(), "numa_node_of_gpu_rank0": numa_node,
                       "streams_on_own_hw_queue": L.dsvg_ctx_streams_apart(b.ctx),
                       "copy_stream_queue": {0: "own", 2: "own (lowest-priority stream)", 3: "own (highest-priority stream)", 1: "shares the analysis stream's", -1: "as the runtime placed it"}.get(L.dsvg_ctx_copy_queue(b.ctx), "?"),
                       "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                       "pictures_without_reconstruction_per_step_rank0": dropped_per_step,
                       "pictures_without_reconstruction_note": "the last picture of a closed GOP is a reference picture nobody predicts from: the reference encoder "
                                                               "reconstructs it and never reads it (dsv_encoder.c:665-708); here it is coded without the inverse "
                                                               "transform -- same packets (bit_exact_timed_output); DSV1_RECON_ALL=1 reconstructs every picture"},
            "bit_exact_vs_cpu": bit_exact,
            "bit_exact_timed_output": timed_check,
            "roofline": kinfo,
            "cpu_baseline": cpu,
        }
        tp = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tp):
            # the whole step against the HBM roof: bytes every kernel of one frame-step batch moved by the counters (the committed
            # rocprofv3 --pmc passes over this command, all kernels summed, scaled to this run's GOPs) / this run's step time
            T = json.load(open(tp))
            st_ = T.get("step")
            if st_:
                hb = st_["hbm_bytes"] * args.gops / T["gops"]
                res["pipeline"] = {"bound": "hbm", "hbm_bytes_per_step": round(hb), "hbm_bytes_per_step_raw": round(st_["hbm_bytes_raw"] * args.gops / T["gops"]),
                                   "achieved": round(hb / (1e-3 * res["ms_per_step"]) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": round(hb / (1e-3 * res["ms_per_step"]) / 1e9 / HBM_PEAK_GBS, 4),
                                   "algorithmic_bytes_per_step": round(41.2 * GOP * W * H * args.gops),
                                   "traffic_stale": traffic_stamp(T)["traffic_stale"], "traffic_commit": T.get("commit", "unstamped"),
                                   "note": "counter bytes = (2 x FETCH_SIZE + WRITE_SIZE) of every kernel of a step (profiles/pmc_traffic.json, "
                                           "FETCH_SIZE tallies 128-byte requests at 64 bytes: profiles/r03_fetch_calib.txt); algorithmic = SURVEY 8(d)'s 41.2 B per luma pixel of the "
                                           "unfused reference pipeline -- the fused kernels move less than that"}
                # the same step against the VALU issue roof: wave64 instructions of every kernel of a step (SQ_INSTS_VALU) / the measured
                # issue rate of the integer / byte / packed forms these kernels are made of -- the step's other roof, and which one binds
                vi = st_.get("valu_insts")
                if vi is None:
                    vi = sum(e.get("valu_insts_per_launch", 0.0) * e.get("launches", 0) for k, e in T["kernels"].items()
                             if not k.startswith("__amd") and k != "k_spin") / max(1, st_.get("steps_profiled", 1))
                if vi:
                    vi = vi * args.gops / T["gops"]
                    vms = vi / (VALU_PEAK_GI * 1e9) * 1e3
                    hms = hb / (6300.0 * 1e9) * 1e3
                    res["pipeline"]["valu"] = {"wave_instr_per_step": round(vi), "peak": VALU_PEAK_GI, "unit": "G wave-instr/s", "ms_at_peak": round(vms, 3),
                                               "frac": round(vms / res["ms_per_step"], 4), "source": "sum of SQ_INSTS_VALU over the kernels of a step, profiles/pmc_traffic.json"}
                    res["pipeline"]["hbm_ms_at_achievable_6300GBs"] = round(hms, 3)
                    res["pipeline"]["binding_roof"] = "valu" if vms > hms else "hbm"
        if extras:
            # the other shapes of BASELINE.json and the batched decoder, each with its own bit-exact check (measured
            # after the headline; the headline's context is closed first so that every shape has the GPU to itself)
            b.close()
            res["value_host_pinned"] = host_pinned
            shapes = {}
            try:
                shapes["cfg2_1080p_intra"] = dict(shape_bench(pkg, A, dev, 1920, 1080, 0x5, 64, 12, 20, 0x10800001, 12, qp=85, gop=0, rc_mode_cli=1),
                                                  config="1920x1080 4:2:0 -gop0 -qp85 -rc_mode1, 64 streams x 12 frames per step")
                shapes["cfg4_4k_gop12"] = dict(shape_bench(pkg, A, dev, 3840, 2160, 0x5, 16, 12, 16, 0x21600004, 12, qp=85, gop=12, rc_mode_cli=1, scd=0),
                                               config="3840x2160 4:2:0 -gop12 -qp85 -rc_mode1 -scd0, 16 closed GOPs x 12 frames per step")
                shapes["cfg4_8gops"] = dict(shape_bench(pkg, A, dev, 3840, 2160, 0x5, 8, 12, 24, 0x21600004, 12, qp=85, gop=12, rc_mode_cli=1, scd=0),
                                            config="3840x2160 4:2:0 -gop12 -qp85 -rc_mode1 -scd0, 8 closed GOPs x 12 frames per step: one GPU's share of config 4's 64 GOPs on an 8-GPU node")
                shapes["cfg3_4gops"] = dict(shape_bench(pkg, A, dev, W, H, FMT, 4, GOP, 60, 0x10800003, 12, qp=QP, gop=GOP, rc_mode_cli=1),
                                            config="1920x1080 4:2:0 -gop12 -qp85 -rc_mode1, 4 closed GOPs x 12 frames = 48 frames per step: SURVEY 8(d)'s config 3 verbatim (the small-batch regime)")
                shapes["cfg5_4k_444_abr"] = dict(shape_bench(pkg, A, dev, 3840, 2160, 0x0, 2, 30, 12, 0x21600005, 6, qp=85, gop=30, rc_mode_cli=0, kbps=20000),
                                                 config="3840x2160 4:4:4 -gop30 -qp85 -rc_mode0 -kbps20000 (ABR: every quantiser from the packet before, rate control on the device), 2 streams x 30 frames per step")
                # config 5 at replica scale (ABR streams are "replicas only" -- several independent streams side by side are how that config fills a chip)
                for nst in (8, 16):
                    shapes["cfg5_abr_x%d" % nst] = dict(shape_bench(pkg, A, dev, 3840, 2160, 0x0, nst, 30, 4, 0x21600005, 0, qp=85, gop=30, rc_mode_cli=0, kbps=20000),
                                                        config="3840x2160 4:4:4 -gop30 -qp85 -rc_mode0 -kbps20000, %d independent ABR streams x 30 frames per step (same clip in every stream; bytes checked on the 2-stream shape)" % nst)
                # the headline's shape and batch on MIXED content: 16 distinct clips of five styles dealt over the 320 GOPs (verdict round 5: the timed batch is 4 clips of one style)
                mix = [0, 1, 2, 4, 7, 0, 1, 2, 4, 7, 0, 1, 2, 4, 0, 0]
                shapes["headline_mixed16"] = dict(shape_bench(pkg, A, dev, W, H, FMT, args.gops, GOP, 6, 0x10800003, 12, style=0, styles=mix, qp=QP, gop=GOP, rc_mode_cli=1),
                                                  config="1920x1080 4:2:0 -gop12 -qp85 -rc_mode1 (the headline's flags), %d closed GOPs x 12 frames per step from 16 distinct clips of clip styles %s "
                                                         "(0 pan + texture, 1 / 4 + flat moving objects: intra blocks, 2 static + textured square, 7 + per-pixel noise)" % (args.gops, mix))
                # the content that leaves the lean kernels: flat moving objects force a third of the blocks intra (whole-grid
                # k_fwd_mc_pix, k_mc for the intra blocks, dense symbols) -- same shape and batch as the headline
                wc = A.gen_clip(W, H, FMT, 0x10800003, 4, style=4)
                shapes["cfg3_worstcase"] = dict(shape_bench(pkg, A, dev, W, H, FMT, args.gops, GOP, 6, 0x10800003, 12, style=4, qp=QP, gop=GOP, rc_mode_cli=1, scd=0),
                                                       config="1920x1080 4:2:0 -gop12 -qp85 -rc_mode1 -scd0, %d closed GOPs x 12 frames per step, clip style 4 "
                                                              "(pan + texture with a flat square of a third of the height and a flat band over the bottom quarter, both changing every frame)" % args.gops,
                                                       intra_blocks_pct_of_P_pictures=intra_block_pct(A, wc, W, H, FMT, qp=QP, gop=GOP, rc_mode_cli=1, scd=0))
                # the floor of the sparse kernels (verdict round 4): strong per-pixel noise that is new in every frame at -qp95 -- nearly every 8x8
                # patch of every P picture carries level-1 symbols (the headline clip flags 5 % of its luma patches); same shape and batch
                shapes["dense_residual"] = dict(shape_bench(pkg, A, dev, W, H, FMT, args.gops, GOP, 6, 0x10800003, 12, style=7, count_patches=True, qp=95, gop=GOP, rc_mode_cli=1, scd=0),
                                                config="1920x1080 4:2:0 -gop12 -qp95 -rc_mode1 -scd0, %d closed GOPs x 12 frames per step, clip style 7 "
                                                       "(the headline's pan + texture under per-pixel noise of +-24 luma / +-12 chroma that changes every frame)" % args.gops)
                shapes["decode_1080p_batched"] = dict(decode_bench(pkg, A, dev, 64, 2),
                                                      config="1920x1080 4:2:0 GOP=12 stream, dsv1_decbatch_*: 64 streams side by side, one picture of each per call")
                if link and "ms_per_step" in shapes["cfg2_1080p_intra"]:
                    # config 2 hands the caller 239 MB of packets per step: its floor is that egress over the link (device -> host)
                    c2 = shapes["cfg2_1080p_intra"]
                    c2["egress_GBs"] = round(c2["dsv_bytes_per_step"] / (c2["ms_per_step"] * 1e-3) / 1e9, 2)
                    c2["link_d2h_GBs"] = link["d2h_GBs"]
                    c2["egress_frac_of_link"] = round(c2["egress_GBs"] / link["d2h_GBs"], 3)
            except Exception as e:                       # the headline stands on its own
                shapes["error"] = repr(e)
            res["shapes"] = shapes
            res["link"] = link
    b.close()
    # BASELINE config 4 (64 closed 4K GOPs over the node's GPUs): runs sharded over the ranks whenever there is more than one
    # (every rank takes part; the headline's context is closed first so the leg has each GPU to itself)
    if (world > 1 or args.cfg4_sharded) and args.full and args.cfg4_gops > 0 and not args.no_extras and args.input == "hbm":
        try:
            c4 = cfg4_sharded(pkg, A, shard, torch, dist, dev, rank, world, shared, max(2, min(args.steps, 4)), args.cfg4_gops)
        except Exception as e:                               # the headline stands on its own
            c4 = {"error": repr(e)}
        if rank == 0:
            res["cfg4_sharded"] = c4
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
