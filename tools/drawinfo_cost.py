#!/usr/bin/env python3
"""What the decoders' debug overlay costs the batched decoder: 64 streams of 1920x1080 4:2:0, GOP 12, device output, packed planar, in
three configurations on the same box in the same session --
    off            this tree's library, dsv1_decbatch_set_draw_info never called
    off, parent    the parent commit's library (--parent-lib PATH: a libdsv1_mi355x.so built from the commit before; left out without)
    on, mode 7     this tree's library, dsv1_decbatch_set_draw_info(7)
-- each in a process of its own (one library per process), the configurations alternating round by round so that drift hits all of
them alike.  "off" costing nothing means: the two off columns differ by no more than either one's own spread from round to round.
    python tools/drawinfo_cost.py [--parent-lib PATH] [--rounds 5] > profiles/drawinfo_cost.txt
The worker (--worker LIB STREAM MODE) binds the C ABI of LIB directly: the package always loads its own library."""
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FMT, N, S = 1920, 1080, 0x5, 24, int(os.environ.get("DEC_STREAMS", "64"))


class Meta(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "subsamp", "fps_num", "fps_den", "aspect_num", "aspect_den")]


class Buf(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("len", C.c_uint)]


def split_packets(stream):
    pk, o = [], 0
    while o + 14 <= len(stream):
        nxt = int.from_bytes(stream[o + 10:o + 14], "big")
        pk.append(stream[o:o + (nxt if nxt else 14)])
        o += len(pk[-1])
    return pk


def worker(lib_path, stream_path, mode, runs=7, warm=2):
    L = C.CDLL(lib_path)
    L.dsvg_last_error.restype = C.c_char_p
    L.dsv1_decbatch_open.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Meta), C.c_int]
    L.dsv1_decbatch_decode.argtypes = [C.c_void_p, C.POINTER(Buf), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    L.dsv1_decbatch_close.argtypes = [C.c_void_p]
    L.dsv1_decbatch_ctx.restype = C.c_void_p
    L.dsv1_decbatch_ctx.argtypes = [C.c_void_p]
    L.dsvg_dev_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    L.dsvg_ctx_sync.argtypes = [C.c_void_p]
    with open(stream_path, "rb") as f:
        pk = [p for p in split_packets(f.read()) if p[5] & 4]
    keep = [(C.c_uint8 * (len(p) + 16)).from_buffer_copy(bytes(p) + b"\0" * 16) for p in pk]
    calls = []
    for k, p in enumerate(pk):
        bufs = (Buf * S)()
        for s in range(S):
            bufs[s].data = C.cast(keep[k], C.POINTER(C.c_uint8))
            bufs[s].len = len(p)
        calls.append(bufs)
    m = Meta(W, H, FMT, 30, 1, 1, 1)
    d = C.c_void_p(None)
    assert L.dsv1_decbatch_open(C.byref(d), 0, C.byref(m), S) == 0, L.dsvg_last_error()
    if mode:
        L.dsv1_decbatch_set_draw_info.argtypes = [C.c_void_p, C.c_int]
        assert L.dsv1_decbatch_set_draw_info(d, mode) == 0
    fb = W * H * 3 // 2
    dst = C.c_void_p(None)
    assert L.dsvg_dev_alloc(L.dsv1_decbatch_ctx(d), C.byref(dst), fb * S) == 0
    status, fnum = (C.c_int * S)(), (C.c_uint32 * S)()
    times = []
    for r in range(warm + runs):
        L.dsvg_ctx_sync(L.dsv1_decbatch_ctx(d))
        t0 = time.perf_counter()
        for bufs in calls:
            assert L.dsv1_decbatch_decode(d, bufs, dst, fb, 1, status, fnum) == 0, L.dsvg_last_error()
        L.dsvg_ctx_sync(L.dsv1_decbatch_ctx(d))
        if r >= warm:
            times.append((time.perf_counter() - t0) / len(calls) * 1e3)
    L.dsvg_ctx_sync(L.dsv1_decbatch_ctx(d))
    L.dsv1_decbatch_close(d)
    print("%.4f %.4f %.4f" % (statistics.median(times), min(times), max(times)))


def main(argv):
    if argv[:1] == ["--worker"]:
        return worker(argv[1], argv[2], int(argv[3]))
    parent = argv[argv.index("--parent-lib") + 1] if "--parent-lib" in argv else None
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import importlib
    import numpy as np
    import _cabi as A
    pkg = importlib.import_module("digital-subband-video-1_amd")
    clip = A.gen_clip(W, H, FMT, 0x10800003, 12, style=1)
    stream = bytes(pkg.encode_clip(np.concatenate([clip] * (N // 12), axis=0), W, H, FMT, qp=85, gop=12, rc_mode_cli=1))
    configs = [("off", pkg.SO_PATH, 0)] + ([("off, parent commit", parent, 0)] if parent else []) + [("on, mode 7", pkg.SO_PATH, 7)]
    res = {name: [] for name, _, _ in configs}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "s.dsv")
        with open(path, "wb") as f:
            f.write(stream)
        for r in range(rounds):
            for name, lib, mode in configs:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib, path, str(mode)], stdout=subprocess.PIPE,
                                     check=True, timeout=300).stdout.decode().split()
                res[name].append(tuple(float(x) for x in out))
    print("batched decoder, %d streams %dx%d 4:2:0 GOP 12, %d picture calls per run (22 with P pictures), device output, packed planar;" % (S, W, H, N))
    print("per round and configuration a process of its own: 7 runs after 2 warm-up runs, median ms per call; %d rounds, alternating" % rounds)
    for name, _, _ in configs:
        med = [t[0] for t in res[name]]
        print("  %-20s %7.3f ms per call (median of the rounds' medians; rounds %s; any run %.3f .. %.3f)" %
              (name, statistics.median(med), " ".join("%.3f" % x for x in med), min(t[1] for t in res[name]), max(t[2] for t in res[name])))
    if not parent:
        print("  (no --parent-lib given: the parent commit's column is left out)")


if __name__ == "__main__":
    main(sys.argv[1:])
